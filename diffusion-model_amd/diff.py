"""Drop-in ``diff`` module: the DDPM scheduler and samplers of the reference
(reference diff.py:10-369) running on the MI355X-native engine.

Call surface, defaults, exception types and RNG draw order are the reference's.
What changes is where the work happens:

* ``denoise_cond`` with CFG on a dmx network batches the uncond/cond forwards into
  one 2B-sample native forward and fuses out-head + CFG mix + DDPM update into one
  kernel (libdmx ``dmx_step``); any other (duck-typed) model is called exactly like
  the reference and only the update runs natively (``dmx_ddpm_update``).
* ``noise_source``:
    - ``"host"`` (default): every Gaussian draw comes from the global torch CPU
      generator in the reference's order (optional encode draw, x_T, one draw per
      step) and is copied to the device — results match the reference PyTorch-CPU
      path on identical seeds;
    - ``"device"``: counter-based Philox on the GPU keyed by (seed, t, global sample
      index); the T loop then runs as replayed hipGraphs with no host round trip.
* Schedule tables are built on the host with the reference's fp32 torch ops, so
  the per-t coefficients are bit-identical to the reference CPU path.
* Few-step sampling (not in the reference): ``sample_latent_cond(..., sampler="ddim",
  steps=S, eta=...)`` runs S strided DDIM steps through the same native step and graph
  loop (``ddim_timesteps`` / ``ddim_tables`` / ``ddim_step``); the defaults leave the
  DDPM path untouched.  ``sampler="dpmpp_2m"`` runs DPM-Solver++(2M) over timesteps uniform in
  log-SNR through the same step and loop (``dpm_timesteps`` / ``dpm_tables`` / ``dpm_step``).
* Image-conditioned sampling (not in the reference): ``sample_latent_cond(..., init_latent=z0,
  mask=m, strength=s)`` starts any of the three samplers from z0 noised to an intermediate
  position (img2img) and / or holds the latent outside ``m`` on z0's forward trajectory after
  every step (inpainting; ``known_tables``, libdmx ``dmx_known_blend``).
* Guidance controls (not in the reference): ``sample_latent_cond(..., guidance_interval=(t_lo, t_hi),
  guidance_rescale=phi)`` applies CFG only to the steps whose timestep lies in the interval — the others
  are one conditional forward — and scales the guided prediction to the conditional one's per-sample
  standard deviation (libdmx ``dmx_step_guided`` / ``dmx_cfg_rescale``).
* Geometry guidance (not in the reference): ``sample_latent_cond(..., geom_scale=s)`` adds the input
  gradient of the GeomHead's masked regression loss against the call's own condition to every step's
  guided prediction (classifier guidance; libdmx ``dmx_step_geom`` / ``dmx_geom_mix``).
* v-prediction (not in the reference): ``Diffuser(..., prediction="v")`` reads the network's output as the
  velocity v = sqrt(ab_t) noise - sqrt(1 - ab_t) x0.  Every sampling entry mixes in output space, converts once
  (eps = sqrt(ab_t) v + sqrt(1 - ab_t) x_t, in the native tail; ``dmx_model_set_prediction`` /
  ``dmx_pred_to_eps``) and runs the eps-form update; ``training_loss`` regresses on v.
* Zero-terminal-SNR schedules (not in the reference): ``Diffuser(prediction="v", zero_terminal_snr=True)`` rescales
  the schedule so that ab_T = 0 (Lin et al. 2023) and runs every update in x0-form — the native tail converts to
  x0 = sqrt(ab_t) x_t - sqrt(1 - ab_t) v and eps and updates without a division
  (``dmx_model_set_prediction_x0``); ``x0_form=True`` does so on any v-schedule.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
import queue
import sys
import threading
from typing import Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch
from tqdm import tqdm

_ROOT = os.path.dirname(os.path.abspath(__file__))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

from dmx import engine as _engine  # noqa: E402

KEY_ORDER = ["x1", "y1", "x2", "y2", "cx", "cy", "cr", "ax", "ay", "ar", "theta1", "theta2"]
CLASS_KEYS = {1: ["x1", "y1", "x2", "y2"], 2: ["cx", "cy", "cr"], 3: ["ax", "ay", "ar", "theta1", "theta2"]}


def _native_kind(model) -> int:
    """libdmx kind of a dmx drop-in network, 0 for foreign (duck-typed) models."""
    return int(getattr(type(model), "_dmx_kind", 0)) if hasattr(model, "native") else 0


class _NoisePrefetch:
    """The next `n` per-step noise draws of a sampler chunk, made on a helper thread from the
    global CPU generator — in the reference's order, nothing else draws meanwhile — into pinned
    buffers, so the host draw (~2 ms at B=64, single-threaded in torch) overlaps the GPU step
    instead of preceding it.  torch.randn(shape, out=buf) consumes the generator exactly like
    torch.randn(shape)."""

    def __init__(self, shape, n: int, depth: int = 2, rows=None):
        self.shape, self.n = tuple(int(v) for v in shape), int(n)
        self.rows = rows  # (start, end): only these rows of each draw go to the device (a rank's shard)
        self.bufs = [torch.empty(self.shape, pin_memory=True) for _ in range(depth + 2)]
        self.events = [None] * len(self.bufs)
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self.err = None
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        try:
            for k in range(self.n):
                j = k % len(self.bufs)
                if self.events[j] is not None:
                    self.events[j].synchronize()  # the H2D copy that last read this buffer is done
                torch.randn(self.shape, out=self.bufs[j])
                self.q.put(k)
        except BaseException as e:  # surfaced to the consumer
            self.err = e
            self.q.put(-1)

    def next(self, device):
        k = self.q.get()
        if k < 0:
            raise self.err
        j = k % len(self.bufs)
        src = self.bufs[j] if self.rows is None else self.bufs[j][self.rows[0]:self.rows[1]]
        out = src.to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self.events[j] = ev
        return out

    def close(self):
        while self.thread.is_alive():  # the consumer stopped early: let the producer finish its draws
            try:
                self.q.get(timeout=0.05)
            except queue.Empty:
                pass
        self.thread.join()


@dataclasses.dataclass
class TrainingLoss:
    """What Diffuser.training_loss returns: `loss` carries the graph (requires_grad when the model
    trains); the rest is detached, for logging and for replaying the batch."""
    loss: torch.Tensor                     # 0-dim: noise_loss + geom_lambda * geom_loss
    noise_loss: torch.Tensor               # 0-dim
    geom_loss: torch.Tensor                # 0-dim (0 without a geometry term)
    per_sample: torch.Tensor               # (B,) weighted noise losses
    t: torch.Tensor                        # (B,) the timesteps used
    drop: torch.Tensor                     # (B,) bool: rows trained as unconditional
    eps: torch.Tensor                      # the network's prediction on the noised latent (a v-model's: v)
    geom: Optional[torch.Tensor]           # the GeomHead's output, None without one
    target: Optional[torch.Tensor] = None  # what eps is regressed on: `noise` itself, or a v-model's
                                           # sqrt(ab_t) noise - sqrt(1 - ab_t) z


@dataclasses.dataclass
class _SamplerPlan:
    """What a sampling call's steps have in common, derived once (Diffuser._plan; the public one-step
    entries fill in the fields they need): the loops of the single-process and the sharded sampler
    walk the same plan, a shard's being the plan of its rows."""
    rule: str                              # "ddpm", "ddim", "dpm" or "invert"
    start: int = 0                         # the loop counter's first value: T, S, p0 of a known-region or
                                           # start-latent loop, or the row count N of an inversion
    tables: Optional[tuple] = None         # coef_tables (ddpm)
    sched: Optional[tuple] = None          # ddim_tables / dpm_tables (the strided rules) / invert_tables
    draws: bool = True                     # do the steps draw noise (ddpm, or ddim with eta > 0)
    scale: float = 0.0                     # guidance scale of the guided steps (0 in a composed plan)
    rescale: float = 0.0                   # CFG rescale phi of the guided steps
    run_g: object = True                   # guided positions: True (all), (p_lo, p_hi) or None (_guided_run)
    known: Optional[tuple] = None          # the known-region blend's operands (engine.known_blend)
    compose: Optional[tuple] = None        # the composed step's branch tables, contiguous on the device
    geom: Optional[tuple] = None           # geometry guidance: (scale row (B,), sig table) on the device
    perturb: Optional[Tuple[int, int]] = None  # perturbed-attention guidance: (blocks, branches) bit masks of compose
    rows: Optional[Tuple[int, int]] = None  # a shard: the rows [s, e) of the global batch
    x_start: Optional[torch.Tensor] = None  # the latent the loop starts from
    cache: int = 1                         # feature caching: a refresh step every cache-th position of a guard
                                           # chunk, reuse steps between (1: every step is the plain step)

    def guided(self, i: int) -> bool:
        return self.run_g is True or (self.run_g is not None and self.run_g[0] <= i <= self.run_g[1])

    def segments(self, i_from: int, i_to: int):
        """Positions i_from .. i_to + 1 cut where the step kind changes: (a, b, guided) pieces."""
        if self.run_g is True:
            return [(i_from, i_to, True)]
        return Diffuser._guidance_segments(i_from, i_to, self.run_g)

    def guidance(self, guided: bool) -> float:
        return self.scale if guided else 0.0

    def new_hist(self, x):
        """The DPM solver's history buffer for x (the loop's first position does not read it), or an
        inversion's source latent: x's values, the loop starting with x == src."""
        if self.rule == "invert":
            return x.detach().to(torch.float32).contiguous().clone()
        return torch.empty_like(x, dtype=torch.float32) if self.rule == "dpm" else None

    def kwargs(self, guided: bool, hist=None, seed=None, use_graph=None, phase: int = 0) -> dict:
        """The keywords of NativeModel.step (seed: a drawn Philox seed, else none) and, with
        use_graph given, NativeModel.sample_loop for a guided or unguided step: a feature that
        is off passes no keyword.  phase: how far into its guard chunk the step (the loop's first
        step) stands — read by a cached plan alone."""
        kw = {}
        if self.cache > 1:
            kw["cache"] = (self.cache, int(phase))
        if seed is not None:
            kw["seed"] = seed
        if use_graph is not None:
            kw["use_graph"] = use_graph
            if self.rows is not None:
                kw["sample_offset"] = self.rows[0]
        if self.rule == "invert":  # (its seed is not read, and it takes none of the parts below)
            kw["invert"] = (self.sched, hist)
            return kw
        if self.sched is not None:
            kw["sched"] = self.sched
        if hist is not None:
            kw["hist"] = hist
        if self.known is not None:
            kw["known"] = self.known
        if guided and self.rescale > 0:
            kw["rescale"] = self.rescale
        if self.compose is not None:
            kw["compose"] = self.compose
        if self.perturb is not None:
            kw["perturb"] = self.perturb
        if guided and self.geom is not None:
            kw["geom"] = self.geom
        return kw


class Diffuser:
    PREDICTIONS = ("eps", "v")

    def __init__(self, num_timesteps=1000, beta_start=0.0001, beta_end=0.02, device="cpu", *, prediction="eps",
                 zero_terminal_snr=False, x0_form=None):
        """prediction (not in the reference): what the network's output means.  "eps": the noise, as the
        reference trains it.  "v": the velocity v = sqrt(ab_t) noise - sqrt(1 - ab_t) x0 (Salimans & Ho
        2022).  A checkpoint does not record it, so the caller states it.  With "v" every sampling entry
        mixes in output space (CFG, composition, perturbed branch, CFG rescale — whose standard deviations
        are then v's — and geometry guidance), converts once, eps = sqrt(ab_t) out + sqrt(1 - ab_t) x_t,
        and runs the eps-form update; training_loss regresses on v.

        zero_terminal_snr (not in the reference): the linear schedule rescaled by Algorithm 1 of Lin et al.
        2023 ("Common diffusion noise schedules and sample steps are flawed") so that ab_T = 0 exactly: the
        last step is pure noise, in training as in sampling.  sqrt(ab) is shifted and scaled in fp32 on the
        CPU so that its first entry keeps its bits and its last becomes 0; alphas = ab_t / ab_{t-1} and
        betas = 1 - alphas follow from the rescaled ab, which is the table every other table is built from
        (it is not re-multiplied from the alphas).  Needs num_timesteps >= 2 and prediction="v": an eps
        prediction at pure noise carries no information.

        x0_form: a v-model's updates written on (x0, eps), x0 = sqrt(ab_t) x_t - sqrt(1 - ab_t) out, with
        no division (x0_tables; include/dmx.h dmx_model_set_prediction_x0) — the eps-form divides by
        sqrt(ab_t), which is 0 at t = T of a zero-terminal-SNR schedule and already ill-conditioned just below
        it.  None: equal to zero_terminal_snr.  True is allowed with any v-schedule; False with
        zero_terminal_snr is refused.  The x0-form DDPM rule takes alpha_bar_prev = 1 at t = 1 in denoise too:
        the wrap-around of the reference's unconditional denoise (coef_tables(clamp_prev=False)) is an
        eps-mode parity quirk and is not carried over.  Only native models take the x0-form."""
        if not isinstance(prediction, str) or prediction not in self.PREDICTIONS:
            raise ValueError(f'prediction must be "eps" or "v" (got {prediction!r})')
        zero_terminal_snr = bool(zero_terminal_snr)
        if x0_form is None:
            x0_form = zero_terminal_snr
        x0_form = bool(x0_form)
        if zero_terminal_snr and prediction != "v":
            raise ValueError('zero_terminal_snr needs prediction="v": eps at pure noise carries no information')
        if x0_form and prediction != "v":
            raise ValueError('x0_form needs prediction="v"')
        if zero_terminal_snr and not x0_form:
            raise ValueError("zero_terminal_snr needs the x0-form: the eps-form update divides by sqrt(ab_T) = 0")
        if zero_terminal_snr and int(num_timesteps) < 2:
            raise ValueError(f"zero_terminal_snr needs num_timesteps >= 2 (got {num_timesteps})")
        self.prediction = prediction
        self.zero_terminal_snr = zero_terminal_snr
        self.x0_form = x0_form
        # diff.py:11-16, evaluated on the CPU (torch's CPU cumprod accumulates in double)
        self.num_timesteps = num_timesteps
        self.device = device
        betas = torch.linspace(beta_start, beta_end, num_timesteps)
        alphas = 1 - betas
        alpha_bars = torch.cumprod(alphas, dim=0)
        if zero_terminal_snr:  # Lin et al. 2023, Algorithm 1, in fp32
            s = torch.sqrt(alpha_bars)
            s1, sT = s[0].clone(), s[-1].clone()
            s = (s - sT) * s1 / (s1 - sT)
            s[0] = s1  # ((s1 - sT) s1 / (s1 - sT) may round off s1: the first entry keeps its bits)
            alpha_bars = s * s
            alpha_bars[0] = torch.cumprod(alphas, dim=0)[0]
            alphas = torch.cat([alpha_bars[:1], alpha_bars[1:] / alpha_bars[:-1]])
            betas = 1 - alphas
        self.betas = betas.to(device)
        self.alphas = alphas.to(device)
        self.alpha_bars = alpha_bars.to(device)
        self._host = (alphas, alpha_bars)
        self._tables: Dict[Tuple[str, bool], Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = {}
        self.noise_source = "host"
        self.use_graph = True
        self.range_fallbacks = 0  # chunks recomputed in fp32 by the range guard

    # ---- schedule tables (per t-1) ---------------------------------------------------------
    def coef_tables(self, device, clamp_prev: bool = True):
        """(c1, c2, sd) with c1 = (1-a)/sqrt(1-ab), c2 = sqrt(a), sd = posterior std.

        clamp_prev=True follows denoise_cond (diff.py:144), False follows denoise's
        wrap-around ``alpha_bars[t_idx-1]`` (diff.py:39)."""
        key = (str(device), clamp_prev)
        if key not in self._tables:
            a, ab = self._host
            idx = torch.arange(self.num_timesteps)
            prev = torch.clamp(idx - 1, min=0) if clamp_prev else idx - 1
            abp = ab[prev]
            c1 = (1 - a) / torch.sqrt(1 - ab)
            c2 = torch.sqrt(a)
            sd = torch.sqrt((1 - a) * (1 - abp) / (1 - ab))
            self._tables[key] = tuple(v.contiguous().to(device) for v in (c1, c2, sd))
        return self._tables[key]

    # ---- strided (DDIM) schedule: one row per position p = 1..S, index p-1 ---------------------
    def ddim_timesteps(self, steps: int) -> List[int]:
        """The S = `steps` timesteps of the strided sampler, ascending: tau_i = ceil(i T / S), i = 1..S
        (tau_S = T; S = T gives 1..T)."""
        T, S = int(self.num_timesteps), int(steps)
        if not 1 <= S <= T:
            raise ValueError(f"steps must be in [1, {T}] (got {steps})")
        return [(i * T + S - 1) // S for i in range(1, S + 1)]

    def ddim_tables(self, steps: int, eta: float = 0.0, device="cpu"):
        """(t_map, k_e, k_a, k_s, k_d, k_n) of the DDIM step (Song et al. 2021, eq. 12) from
        t = tau_p to s = tau_{p-1} (tau_0 = 0, alpha_bar 1), per position p at index p-1:
        k_e = sqrt(1-ab[t]), k_a = sqrt(ab[t]), k_s = sqrt(ab[s]),
        k_n = sigma = eta sqrt((1-ab[s])/(1-ab[t])) sqrt(1-ab[t]/ab[s]), k_d = sqrt(max(1-ab[s]-sigma^2, 0)),
        so that x0 = (x - k_e eps)/k_a and x' = k_s x0 + k_d eps + k_n noise.  Computed in float64 from
        the fp32 alpha_bars and rounded to fp32 once; cached per (steps, eta, device)."""
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta must be in [0, 1] (got {eta})")
        key = (int(steps), eta, str(device))
        cache = self.__dict__.setdefault("_ddim_tables", {})
        if key not in cache:
            tau = self.ddim_timesteps(steps)
            ab = torch.cat([torch.ones(1, dtype=torch.float64), self._host[1].double()])  # ab[0] := 1
            t = torch.tensor(tau, dtype=torch.long)
            s = torch.tensor([0] + tau[:-1], dtype=torch.long)
            ab_t, ab_s = ab[t], ab[s]
            sigma = eta * torch.sqrt((1 - ab_s) / (1 - ab_t)) * torch.sqrt(1 - ab_t / ab_s)
            k_d = torch.sqrt(torch.clamp(1 - ab_s - sigma * sigma, min=0.0))
            tabs = (torch.sqrt(1 - ab_t), torch.sqrt(ab_t), torch.sqrt(ab_s), k_d, sigma)
            cache[key] = (t.contiguous().to(device),) + tuple(v.float().contiguous().to(device) for v in tabs)
        return cache[key]

    # ---- DPM-Solver++(2M) schedule (Lu et al. 2022, Alg. 2): one row per position, as above -------
    DPM_SPACINGS = ("logsnr", "uniform")

    def dpm_timesteps(self, steps: int, spacing: str = "logsnr") -> List[int]:
        """The S = `steps` ascending timesteps of the DPM-Solver++ sampler, tau_S = T.
        "uniform": ddim_timesteps(S).  "logsnr": uniform in lam[t] = 0.5 ln(ab[t] / (1 - ab[t])) between
        lam[1] and lam[T] — each grid point goes to the nearest timestep (ties to the smaller), then a
        forward pass makes the list strictly ascending from tau_1 and a backward pass fits it under
        tau_S = T.  S = 1 gives [T] and S = T gives 1..T.
        On a zero-terminal-SNR schedule lam[T] = -inf: tau_S = T stays, and the other S - 1 points are placed
        the same way between lam[1] and lam[T-1] (a single one at the middle of that range) and fitted under
        T - 1."""
        if spacing not in self.DPM_SPACINGS:
            raise ValueError(f'spacing must be "logsnr" or "uniform" (got {spacing!r})')
        T, S = int(self.num_timesteps), int(steps)
        if not 1 <= S <= T:
            raise ValueError(f"steps must be in [1, {T}] (got {steps})")
        if spacing == "uniform":
            return self.ddim_timesteps(S)
        if S == 1:
            return [T]
        ab = self._host[1].double()
        lam = 0.5 * torch.log(ab / (1 - ab))  # lam[t] at index t - 1, strictly decreasing
        if float(ab[T - 1]) == 0.0:  # lam[T] = -inf: the grid spans lam[1] .. lam[T-1], and T is appended
            lam = lam[:T - 1]
            frac = (torch.arange(S - 1, dtype=torch.float64) / (S - 2) if S > 2
                    else torch.full((1,), 0.5, dtype=torch.float64))
            grid = lam[0] + frac * (lam[T - 2] - lam[0])
            tau = [int(torch.argmin(torch.abs(lam - g))) + 1 for g in grid] + [T]
        else:
            grid = lam[0] + torch.arange(S, dtype=torch.float64) / (S - 1) * (lam[T - 1] - lam[0])
            # argmin returns the first minimum: ties go to the smaller t
            tau = [int(torch.argmin(torch.abs(lam - g))) + 1 for g in grid]
        for i in range(1, S):
            tau[i] = max(tau[i], tau[i - 1] + 1)
        tau[S - 1] = T
        for i in range(S - 2, -1, -1):
            tau[i] = min(tau[i], tau[i + 1] - 1)
        return tau

    def dpm_tables(self, steps: int, spacing: str = "logsnr", device="cpu", start: Optional[int] = None):
        """(t_map, k_e, k_a, k_x, k_c, k_p) of the DPM-Solver++(2M) step from t = tau_p to s = tau_{p-1}
        (tau_0 = 0, alpha_bar 1), u = tau_{p+1} being the step before, per position p at index p-1:
        k_e = sqrt(1-ab[t]), k_a = sqrt(ab[t]), k_x = sqrt(1-ab[s]) / sqrt(1-ab[t]),
        m = sqrt(ab[s]) - k_x sqrt(ab[t]) (= -alpha_s expm1(-h), h = lam[s] - lam[t]); first-order rows
        (p = S and p = 1): k_c = m, k_p = 0; otherwise r = (lam[t] - lam[u]) / (lam[s] - lam[t]),
        k_c = m (1 + 1/(2r)), k_p = -m / (2r); so that x0 = (x - k_e eps)/k_a and
        x' = k_x x + k_c x0 + k_p hist.  Computed in float64 from the fp32 alpha_bars and rounded to fp32
        once; cached per (steps, spacing, device, start).  The result is an engine.DpmSchedule (a tuple).
        start = p0 in [1, S): the schedule of a loop that enters at position p0 (img2img) — row p0 is
        first-order too, so no step reads a history that was never written; the other rows are those
        of start=None.  start = S is start=None.
        On a zero-terminal-SNR schedule the terminal row has k_a = 0, which is correct and which the x0-form
        does not read; the row after it (u = T, lam[u] = -inf, r = inf) is first-order: k_c = m, k_p = +0.0."""
        if start is not None:
            start = int(start)
            if not 1 <= start <= int(steps):
                raise ValueError(f"start must be in [1, {int(steps)}] (got {start})")
            if start == int(steps):
                start = None
        key = (int(steps), str(spacing), str(device)) + ((start,) if start is not None else ())
        cache = self.__dict__.setdefault("_dpm_tables", {})
        if key not in cache:
            tau = self.dpm_timesteps(steps, spacing)
            S = len(tau)
            ab = torch.cat([torch.ones(1, dtype=torch.float64), self._host[1].double()])  # ab[0] := 1
            t = torch.tensor(tau, dtype=torch.long)
            s = torch.tensor([0] + tau[:-1], dtype=torch.long)
            ab_t, ab_s = ab[t], ab[s]
            k_e, k_a = torch.sqrt(1 - ab_t), torch.sqrt(ab_t)
            k_x = torch.sqrt(1 - ab_s) / k_e
            m = torch.sqrt(ab_s) - k_x * k_a
            k_c, k_p = m.clone(), torch.zeros_like(m)
            if S > 2:  # second-order rows 1 < p < S (indices 1 .. S-2)
                lam = 0.5 * torch.log(ab[1:] / (1 - ab[1:]))  # lam[t] at index t - 1
                mid = slice(1, S - 1)
                lt, ls, lu = lam[t[mid] - 1], lam[s[mid] - 1], lam[t[2:] - 1]
                r = (lt - lu) / (ls - lt)
                k_c[mid] = m[mid] * (1 + 1 / (2 * r))
                k_p[mid] = -m[mid] / (2 * r)
                first = torch.isinf(lu)  # the step before started at pure noise: r = inf, first-order
                k_c[mid] = torch.where(first, m[mid], k_c[mid])
                k_p[mid] = torch.where(first, torch.zeros_like(lu), k_p[mid])  # (+0.0, not the -0.0 of -m / inf)
            if start is not None:  # the loop enters here: nothing has written the history yet
                k_c[start - 1], k_p[start - 1] = m[start - 1], 0.0
            tabs = (k_e, k_a, k_x, k_c, k_p)
            cache[key] = _engine.DpmSchedule((t.contiguous().to(device),)
                                             + tuple(v.float().contiguous().to(device) for v in tabs))
        return cache[key]

    # ---- DDIM inversion: R + 1 rows per position p = 1..p0, stored in countdown order -------------
    def invert_tables(self, steps: int, strength=None, refine: int = 0, device="cpu"):
        """(t_eval, i_x, i_e, adv) of the DDIM inversion over the first p0 = _known_start(strength, steps)
        positions of ddim_timesteps(steps), R = `refine` fixed-point refinements per position.  Position p
        goes from s = tau_{p-1} (tau_0 = 0, alpha_bar 1) up to t = tau_p in the rows k = 0..R:
        i_x = sqrt(ab[t]/ab[s]), i_e = sqrt(1-ab[t]) - i_x sqrt(1-ab[s]), so that y = i_x src + i_e eps;
        t_eval = s for k = 0 (tau_1 at p = 1: there is no timestep 0) and t for k >= 1; adv = 1 on row R,
        where y becomes the next position's src.  The N = p0 (R + 1) rows are laid out in countdown
        order: the loop counter c runs N..1 and reads row c - 1, the forward index being j = N - c,
        p = j // (R + 1) + 1, k = j % (R + 1).  int64 / fp32 / fp32 / int32; computed in float64 from the
        fp32 alpha_bars and rounded to fp32 once; cached per (steps, p0, refine, device)."""
        if isinstance(refine, bool) or not isinstance(refine, int) or refine < 0:
            raise ValueError(f"refine must be an int >= 0 (got {refine!r})")
        if isinstance(steps, bool) or not isinstance(steps, int):
            raise ValueError(f"steps must be an int (got {steps!r})")
        tau = self.ddim_timesteps(steps)
        p0, R = self._known_start(strength, len(tau)), refine
        key = (steps, p0, R, str(device))
        cache = self.__dict__.setdefault("_invert_tables", {})
        if key not in cache:
            ab = torch.cat([torch.ones(1, dtype=torch.float64), self._host[1].double()])  # ab[0] := 1
            p = torch.arange(p0 * (R + 1), dtype=torch.long) // (R + 1) + 1
            k = torch.arange(p0 * (R + 1), dtype=torch.long) % (R + 1)
            tau_t = torch.tensor([0] + tau, dtype=torch.long)
            s, t = tau_t[p - 1], tau_t[p]
            i_x = torch.sqrt(ab[t] / ab[s])
            i_e = torch.sqrt(1 - ab[t]) - i_x * torch.sqrt(1 - ab[s])
            t_eval = torch.where(k == 0, torch.clamp(s, min=tau[0]), t)
            rows = (t_eval, i_x.float(), i_e.float(), (k == R).to(torch.int32))
            cache[key] = tuple(v.flip(0).contiguous().to(device) for v in rows)
        return cache[key]

    # ---- known-region sampling (img2img start, masked inpainting): one row per position, as above --
    def known_tables(self, tau, device="cpu"):
        """(q_a, q_e) of the known-region blend for the ascending timesteps `tau` of a loop (tau_p at
        index p-1; the DDPM loop: 1..T): row p-1 holds q_a = sqrt(ab[s]), q_e = sqrt(1 - ab[s]) for
        s = tau_{p-1}, the timestep the step at position p arrives at (tau_0 = 0, ab[0] = 1: row 0 is
        exactly (1, 0)).  Computed in float64 from the fp32 alpha_bars and rounded to fp32 once; cached
        per (tau, device)."""
        tau = tuple(int(v) for v in tau)
        T = int(self.num_timesteps)
        if not tau or tau[0] < 1 or tau[-1] > T or any(b <= a for a, b in zip(tau, tau[1:])):
            raise ValueError(f"tau must be strictly ascending timesteps in [1, {T}]")
        key = (tau, str(device))
        cache = self.__dict__.setdefault("_known_tables", {})
        if key not in cache:
            ab = torch.cat([torch.ones(1, dtype=torch.float64), self._host[1].double()])  # ab[0] := 1
            ab_s = ab[torch.tensor((0,) + tau[:-1], dtype=torch.long)]
            cache[key] = tuple(v.float().contiguous().to(device) for v in (torch.sqrt(ab_s), torch.sqrt(1 - ab_s)))
        return cache[key]

    def _mode_timesteps(self, mode) -> List[int]:
        """tau of a _sampler_mode result: the timesteps its loop's positions 1..S stand for."""
        if mode is None:
            return list(range(1, int(self.num_timesteps) + 1))
        if mode[0] == "invert":  # (its rows walk the first p0 of these upwards)
            return self.ddim_timesteps(mode[1])
        return self.ddim_timesteps(mode[1]) if mode[0] == "ddim" else self.dpm_timesteps(mode[1], mode[2])

    @staticmethod
    def _known_start(strength, S: int) -> int:
        """The position p0 a known-region loop of S positions enters at: S for strength None, otherwise
        min(S, max(1, floor(strength S + 0.5))) for strength in (0, 1]."""
        if strength is None:
            return int(S)
        s = float(strength)
        if not 0.0 < s <= 1.0:
            raise ValueError(f"strength must be in (0, 1] (got {strength})")
        return min(int(S), max(1, int(math.floor(s * int(S) + 0.5))))

    @staticmethod
    def _known_inputs(init_latent, mask, strength, B: int, z_shape):
        """Argument rules of the samplers' (init_latent, mask, strength) keywords -> None without them,
        else (z0, mask or None, strength, (C, h, w)): z0 (B,C,h,w) and mask (B,1,h,w) fp32 contiguous,
        broadcast to the batch.  Every violation raises ValueError."""
        if init_latent is None:
            if mask is not None or strength is not None:
                raise ValueError("`mask` and `strength` need `init_latent`")
            return None
        Diffuser._known_start(strength, 1)
        if not isinstance(init_latent, torch.Tensor) or init_latent.dim() not in (3, 4):
            raise ValueError("init_latent must be a (B,C,h,w), (1,C,h,w) or (C,h,w) tensor")
        z0 = init_latent if init_latent.dim() == 4 else init_latent.unsqueeze(0)
        if z0.shape[0] not in (1, B) or min(z0.shape) < 1:
            raise ValueError(f"init_latent has {z0.shape[0]} samples for a batch of {B}")
        shape = tuple(int(v) for v in z0.shape[1:])
        if z_shape is not None and tuple(int(v) for v in z_shape) != shape:
            raise ValueError(f"init_latent shape {shape} != z_shape {tuple(z_shape)}")
        z0 = z0.detach().to(torch.float32).expand(B, *shape).contiguous()
        if mask is not None:
            h, w = shape[1:]
            if not isinstance(mask, torch.Tensor) or tuple(mask.shape) not in ((B, 1, h, w), (1, 1, h, w), (h, w)):
                raise ValueError(f"mask must be a {(B, 1, h, w)}, {(1, 1, h, w)} or {(h, w)} tensor")
            mask = mask.detach().to(torch.float32).reshape(-1, 1, h, w)
            if not bool(((mask >= 0) & (mask <= 1)).all()):
                raise ValueError("mask values must lie in [0, 1]")
            mask = mask.expand(B, 1, h, w).contiguous()
        return z0, mask, strength, shape

    @classmethod
    def _sampler_mode(cls, sampler, steps, eta, spacing, T):
        """Argument rules of the samplers' (sampler, steps, eta, spacing) keywords ->
        None (DDPM), ("ddim", S, eta) or ("dpm", S, spacing)."""
        if sampler != "dpmpp_2m" and spacing is not None:
            raise ValueError(f'`spacing` belongs to sampler="dpmpp_2m" (got sampler={sampler!r})')
        if sampler not in ("ddpm", "ddim", "dpmpp_2m"):
            raise ValueError(f'sampler must be "ddpm", "ddim" or "dpmpp_2m" (got {sampler!r})')
        if sampler == "ddpm":
            if steps is not None:
                raise ValueError('sampler="ddpm" walks all timesteps and takes no `steps`; strided ancestral '
                                 'sampling is sampler="ddim", eta=1.0')
            return None
        if steps is None or not 1 <= int(steps) <= int(T):
            raise ValueError(f'sampler="{sampler}" needs steps in [1, {T}] (got {steps})')
        if sampler == "ddim":
            if not 0.0 <= float(eta) <= 1.0:
                raise ValueError(f"eta must be in [0, 1] (got {eta})")
            return ("ddim", int(steps), float(eta))
        if float(eta) != 0.0:
            raise ValueError(f'sampler="dpmpp_2m" is deterministic: eta must be 0 (got {eta})')
        spacing = "logsnr" if spacing is None else spacing
        if spacing not in cls.DPM_SPACINGS:
            raise ValueError(f'spacing must be None, "logsnr" or "uniform" (got {spacing!r})')
        return ("dpm", int(steps), spacing)

    # ---- guidance controls: CFG interval and CFG rescale ---------------------------------------
    @staticmethod
    def _guidance_args(guidance_scale, guidance_interval, guidance_rescale, T):
        """Argument rules of the samplers' (guidance_interval, guidance_rescale) keywords ->
        (None or (t_lo, t_hi) ints, phi float).  The interval bounds are network timesteps with
        1 <= t_lo <= t_hi <= T, phi lies in [0, 1], and either control needs guidance_scale > 0.
        Every violation raises ValueError."""
        try:
            phi = float(guidance_rescale)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_rescale must be a number in [0, 1] (got {guidance_rescale!r})") from None
        if not 0.0 <= phi <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"guidance_rescale must be in [0, 1] (got {guidance_rescale})")
        interval = None
        if guidance_interval is not None:
            iv = guidance_interval
            ok = isinstance(iv, (tuple, list)) and len(iv) == 2 and all(
                isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in iv)
            if not ok or not 1 <= int(iv[0]) <= int(iv[1]) <= int(T):
                raise ValueError(f"guidance_interval must be None or ints (t_lo, t_hi) with 1 <= t_lo <= t_hi <= {T} "
                                 f"(got {guidance_interval!r})")
            interval = (int(iv[0]), int(iv[1]))
        if (interval is not None or phi > 0.0) and not (guidance_scale is not None and guidance_scale > 0):
            raise ValueError("guidance_interval / guidance_rescale need guidance_scale > 0 "
                             f"(got guidance_scale={guidance_scale!r})")
        return interval, phi

    # ---- geometry guidance: the GeomHead's input gradient joins the guided prediction -----------
    @classmethod
    def _geom_args(cls, geom_scale, B, model=None, guidance_scale=None, guidance_interval=None,
                   guidance_rescale=0.0, base="null", also=None, cond=None):
        """Argument rules of the samplers' geom_scale keyword -> None (0, or B zeros: the call is the
        plain one) or the (B,) fp32 scale row on the CPU.  geom_scale is a float or B finite floats,
        all >= 0.  A non-zero scale needs a model with a GeomHead (a dmx network must be
        UnetCondWithGeomHead; a foreign model is asked at its first step), a scalar guidance_scale > 0,
        no guidance_interval / guidance_rescale / base / also, and a condition (`cond`) to aim at — a
        row whose mask is all zero is allowed and takes no guidance.  Every violation raises ValueError."""
        row = cls._weight_row(geom_scale, B, "geom_scale")
        if bool((row < 0).any()):
            raise ValueError(f"geom_scale must be >= 0 (got {geom_scale!r})")
        if not bool((row != 0).any()):
            return None
        if model is not None and hasattr(model, "native") and _native_kind(model) != 1:
            raise ValueError("geom_scale needs a model with a GeomHead (UnetCondWithGeomHead)")
        if cls._per_sample(guidance_scale):
            raise ValueError("geom_scale takes a scalar guidance_scale (no per-sample scale)")
        try:
            ok = guidance_scale is not None and float(guidance_scale) > 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"geom_scale needs guidance_scale > 0 (got guidance_scale={guidance_scale!r})")
        try:
            phi = float(guidance_rescale)
        except (TypeError, ValueError):
            phi = float("nan")
        if guidance_interval is not None or phi != 0.0:
            raise ValueError("geom_scale takes no guidance_interval / guidance_rescale")
        if not (isinstance(base, str) and base == "null") or also:
            raise ValueError("geom_scale takes no composed guidance (base / also)")
        if cond is None:
            raise ValueError("geom_scale needs a condition to aim at (cond is None)")
        return row

    def geom_sig(self, device):
        """sqrt(1 - alpha_bar[t]) at index t - 1, fp32 from the fp32 alpha_bars: the sig table of a
        geometry-guided DDPM step (the strided rules use their schedule's k_e, the same quantity per position).
        A v-model's mix happens in output space, where eps += s sig dL/dx reads v += s (sig / sqrt(ab)) dL/dx:
        the table is then sqrt(1 - ab) / sqrt(ab), one fp32 division of the two fp32 roots.  A row with
        ab_t = 0 (the last of a zero-terminal-SNR schedule) gets sig = 0: that one step is not steered — at pure
        noise the latent says nothing about x0, and an eps shift cannot move x0."""
        cache = self.__dict__.setdefault("_geom_sig", {})
        key = (str(device), self.prediction)
        if key not in cache:
            sig = torch.sqrt(1 - self._host[1])
            if self.prediction == "v":
                root = torch.sqrt(self._host[1])
                sig = torch.where(root == 0, torch.zeros_like(sig), sig / root)
            cache[key] = sig.contiguous().to(device)
        return cache[key]

    def _sched_sig(self, sched):
        """geom_sig per position of a strided schedule (t_map, k_e, k_a, ..): k_e, over k_a for a v-model
        (0 where k_a = 0, as in geom_sig)."""
        if self.prediction != "v":
            return sched[1]
        return torch.where(sched[2] == 0, torch.zeros_like(sched[1]), sched[1] / sched[2]).contiguous()

    # ---- what the network predicts -------------------------------------------------------------
    def pred_tables(self, device):
        """(p_o, p_x) = sqrt(ab), sqrt(1 - ab) per t-1: the coefficients of a v-model's conversion
        eps = p_o[t-1] out + p_x[t-1] x_t — the values noise_tables builds on the host, copied to `device`
        (not evaluated a second time there)."""
        host = self.noise_tables("cpu")
        if torch.device(device).type == "cpu":
            return host
        key = ("pred", str(device))
        if key not in self._tables:
            self._tables[key] = tuple(k.to(device) for k in host)
        return self._tables[key]

    def x0_tables(self, device):
        """(d_s, d_d) per t-1: the DDPM posterior mean written on (x0, eps), mu = d_s x0 + d_d eps, with
        d_s = sqrt(ab_prev), d_d = (1 - ab_prev) sqrt(a_t) / sqrt(1 - ab_t) and ab_prev = 1 at t = 1 (row 0 is
        exactly (1, 0)); the posterior sd stays coef_tables' table.  Finite at ab_T = 0, where d_d = 0.
        Computed in float64 from the fp32 alphas and alpha_bars and rounded to fp32 once; cached per device."""
        key = ("x0", str(device))
        if key not in self._tables:
            a, ab = (v.double() for v in self._host)
            abp = torch.cat([torch.ones(1, dtype=torch.float64), ab[:-1]])
            tabs = (torch.sqrt(abp), (1 - abp) * torch.sqrt(a) / torch.sqrt(1 - ab))
            self._tables[key] = tuple(v.float().contiguous().to(device) for v in tabs)
        return self._tables[key]

    def _native(self, model):
        """model.native() with its prediction set to this Diffuser's (a repeated setting costs nothing)."""
        nm = model.native()
        self._set_prediction(nm)
        return nm

    def _set_prediction(self, nm):
        """Tell the native model `nm` this Diffuser's prediction.  A stand-in for NativeModel that knows no
        predictions reads eps: it is left alone in eps-mode and refused in v-mode."""
        setter = getattr(nm, "set_prediction", None)
        if self.prediction == "v":
            if setter is None:
                raise TypeError(f'prediction="v" needs a native model that can be told so ({type(nm).__name__} has '
                                f"no set_prediction)")
            if self.x0_form:  # the x0-form instances: the same conversion tables plus the posterior's
                d_s, d_d = self.x0_tables(nm.device)
                setter("v", *self.pred_tables(nm.device), d_s=d_s, d_d=d_d)
            else:
                setter("v", *self.pred_tables(nm.device))
        elif setter is not None:
            setter("eps")

    def _to_eps(self, eu, ec, g, x, t):
        """A foreign model's operands (eu, ec, g) as eps: unchanged for an eps-model; a v-model's are mixed
        in output space, eu + g (ec - eu) in torch ops (the update's own expression), then converted at the
        network timesteps t on the latent x the model saw (engine.pred_to_eps) -> (eps, None, 0.0)."""
        if self.prediction != "v":
            return eu, ec, g
        if self.x0_form:
            raise TypeError("x0_form needs a native dmx model on the GPU: the stand-alone updates of a foreign "
                            "model are eps-form")
        out = eu if ec is None else eu + g * (ec - eu)
        return _engine.pred_to_eps(out, x, t, *self.pred_tables(x.device)), None, 0.0

    @staticmethod
    def _geom_loss_grad(model, x, t, y, cond_vals, cond_mask):
        """A foreign model's geometry-guidance gradient dL/dx, from torch autograd over its own forward
        (x a leaf, grad mode on): L = sum_n sum_j m_nj (geom_nj - v_nj)^2 / max(sum_j m_nj, 1e-6).  The
        forward must return (eps, geom)."""
        if cond_vals is None or cond_mask is None:
            raise ValueError("geom_scale needs cond_vals and cond_mask")
        with torch.enable_grad():
            xl = x.detach().clone().requires_grad_(True)
            out = model(xl, t, y, cond_vals=cond_vals, cond_mask=cond_mask)
            if not isinstance(out, (tuple, list)) or len(out) < 2 or not isinstance(out[1], torch.Tensor):
                raise ValueError("geom_scale needs a model whose forward returns (eps, geom)")
            m = cond_mask.to(out[1].dtype)
            loss = ((m * (out[1] - cond_vals).pow(2)).sum(-1) / m.sum(-1).clamp_min(1e-6)).sum()
            grad, = torch.autograd.grad(loss, xl)
        return grad.detach()

    # ---- composed guidance: K weighted condition branches over a chosen base -------------------
    COMPOSE_MAX = 4  # extra branches over the base (include/dmx.h DMX_COMPOSE_MAX)

    @staticmethod
    def _per_sample(v) -> bool:
        """Is a guidance scale / weight given per sample (a sequence, an array or a tensor with a dimension)?"""
        return isinstance(v, (list, tuple, np.ndarray)) or (isinstance(v, torch.Tensor) and v.dim() >= 1)

    @classmethod
    def _weight_row(cls, v, B: int, what: str) -> torch.Tensor:
        """A float or B floats -> (B,) fp32 on the CPU; not a finite number, or another length: ValueError."""
        try:
            if cls._per_sample(v):
                row = torch.as_tensor(v).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
            else:
                row = torch.full((B,), float(v), dtype=torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{what} must be a float or {B} floats (got {v!r})") from None
        if row.numel() != B:
            raise ValueError(f"{what} has {row.numel()} entries for {B} samples")
        if not bool(torch.isfinite(row).all()):
            raise ValueError(f"{what} must be finite (got {v!r})")
        return row

    def _compose_args(self, y_list, vals, msk, guidance_scale, base="null", also=None, guidance_interval=None,
                      guidance_rescale=0.0, null_label=0, key_order=None, class_keys=None, device="cpu"):
        """Argument rules of the samplers' (base, also) keywords and of a per-sample guidance_scale ->
        None (the call is the plain one: base "null", no `also`, a scalar scale) or the branch tables
        (y_rows (K+1,B) int64, vals_rows (K+1,B,Kc), mask_rows (K+1,B,Kc), weights (K,B) fp32) on
        `device`.  Branch 0 is the base: "null" = null label with the call's vals / msk, "dropped" = null
        label with vals = mask = 0 (the input the training's joint dropout produced), a condition spec =
        a negative condition.  Branch 1 is the call's own condition with weight guidance_scale (a
        positive float, or B finite floats); branches 2.. are the specs of `also` (at most three).  A
        spec is a dict: "classes" (an int or B ints), optional "cond" / "cond_mask" (every form
        _build_cond takes) and, in `also` only, "weight" (a float or B floats, finite).  Every violation
        raises ValueError; nothing here touches a GPU unless `device` is one."""
        B = len(y_list)
        also = [] if also is None else also
        if not isinstance(also, (list, tuple)):
            raise ValueError(f"`also` must be a list of condition specs (got {type(also).__name__})")
        if isinstance(base, str):
            if base not in ("null", "dropped"):
                raise ValueError(f'base must be "null", "dropped" or a condition spec (got {base!r})')
        elif not isinstance(base, dict):
            raise ValueError(f'base must be "null", "dropped" or a condition spec (got {type(base).__name__})')
        per_sample = self._per_sample(guidance_scale)
        if isinstance(base, str) and base == "null" and not also and not per_sample:
            return None
        if 1 + len(also) > self.COMPOSE_MAX:
            raise ValueError(f"at most {self.COMPOSE_MAX} condition branches: the call's own and "
                             f"{self.COMPOSE_MAX - 1} in `also` (got {len(also)})")
        if guidance_interval is not None:
            raise ValueError("composed guidance (base / also / per-sample guidance_scale) takes no guidance_interval")
        try:
            phi = float(guidance_rescale)
        except (TypeError, ValueError):
            phi = float("nan")
        if phi != 0.0:
            raise ValueError("composed guidance (base / also / per-sample guidance_scale) takes no guidance_rescale")
        if per_sample:
            w1 = self._weight_row(guidance_scale, B, "guidance_scale")
        else:
            try:
                ok = guidance_scale is not None and float(guidance_scale) > 0 and np.isfinite(float(guidance_scale))
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"composed guidance needs guidance_scale > 0 (got {guidance_scale!r})")
            w1 = self._weight_row(guidance_scale, B, "guidance_scale")

        def spec_rows(spec, where, weighted):
            if not isinstance(spec, dict):
                raise ValueError(f"{where}: a condition spec is a dict (got {type(spec).__name__})")
            allowed = {"classes", "cond", "cond_mask"} | ({"weight"} if weighted else set())
            unknown = set(spec) - allowed
            if unknown or "classes" not in spec or (weighted and "weight" not in spec):
                raise ValueError(f"{where}: a condition spec has the keys {sorted(allowed)}, 'classes' "
                                 f"{'and weight ' if weighted else ''}required (got {sorted(map(str, spec))})")
            cl = spec["classes"]
            if isinstance(cl, (int, np.integer)) and not isinstance(cl, bool):
                ys = [int(cl)] * B
            else:
                try:
                    ys = [int(c) for c in (cl.tolist() if isinstance(cl, (torch.Tensor, np.ndarray)) else cl)]
                except (TypeError, ValueError):
                    raise ValueError(f"{where}: 'classes' must be an int or {B} ints (got {cl!r})") from None
                if len(ys) != B:
                    raise ValueError(f"{where}: 'classes' has {len(ys)} entries for {B} samples")
            v, m = self._build_cond(ys, spec.get("cond"), spec.get("cond_mask"), key_order, class_keys, device)
            if tuple(v.shape) != tuple(vals.shape) or tuple(m.shape) != tuple(vals.shape):
                raise ValueError(f"{where}: cond rows {tuple(v.shape)} differ from the call's {tuple(vals.shape)}")
            w = self._weight_row(spec["weight"], B, f"{where}: 'weight'") if weighted else None
            return torch.tensor(ys, dtype=torch.long, device=device), v.float(), m.float(), w

        y_call = torch.tensor([int(c) for c in y_list], dtype=torch.long, device=device)
        v_call, m_call = vals.to(device).float(), msk.to(device).float()
        if isinstance(base, dict):
            y0, v0, m0, _ = spec_rows(base, "base", False)
        else:
            y0 = torch.full_like(y_call, int(null_label))
            v0, m0 = (v_call, m_call) if base == "null" else (torch.zeros_like(v_call), torch.zeros_like(m_call))
        ys, vs, ms, ws = [y0, y_call], [v0, v_call], [m0, m_call], [w1]
        for i, spec in enumerate(also):
            yk, vk, mk, wk = spec_rows(spec, f"also[{i}]", True)
            ys.append(yk), vs.append(vk), ms.append(mk), ws.append(wk)
        return (torch.stack(ys).contiguous(), torch.stack(vs).contiguous(), torch.stack(ms).contiguous(),
                torch.stack(ws).to(device).contiguous())

    # ---- perturbed-attention guidance: one more branch, its self-attention replaced by the identity --
    PAG_BLOCKS = ("sa1", "sa2", "sa3", "sa4", "sa5", "sa6")  # bit i of dmx_perturb.blocks is PAG_BLOCKS[i]

    def _pag_args(self, pag_scale, pag_blocks, y_list, vals, msk, guidance_scale, compose=None, model=None,
                  guidance_interval=None, guidance_rescale=0.0, geom_scale=0.0, null_label=0, device="cpu"):
        """Argument rules of the samplers' (pag_scale, pag_blocks) keywords -> None (pag_scale 0, or B
        zeros: the call is the one without the keywords) or (branch tables, (blocks, branches)): the
        tables of _compose_args with one branch appended — the main condition's rows (branch 1) again,
        which the step runs with identity attention in `pag_blocks` — and the bit masks of
        include/dmx.h dmx_perturb.  pag_scale = s is a float or B finite floats, all >= 0; the appended
        branch has the weight row -s and the main branch's becomes fp32(g + s), so the composed mix
        e_0 + sum_k w_k (e_k - e_0) is e_u + g (e_c - e_u) + s (e_c - e_p).  compose: _compose_args'
        result for the call; None with guidance_scale > 0 stands for the plain CFG call (base "null"),
        and with guidance_scale 0 the composition is K = 1 over the main condition as the base:
        e_c + s (e_c - e_p), at the cost of a CFG step.  pag_blocks is a non-empty collection of names
        from PAG_BLOCKS, none twice.  A non-zero scale needs a conditional dmx network, at most two
        `also` specs, and no guidance_interval / guidance_rescale / geom_scale.  Every violation raises
        ValueError; nothing here touches a GPU unless `device` is one, and nothing is drawn."""
        B = len(y_list)
        row = self._weight_row(pag_scale, B, "pag_scale")
        if bool((row < 0).any()):
            raise ValueError(f"pag_scale must be >= 0 (got {pag_scale!r})")
        if not bool((row != 0).any()):
            return None
        names = [pag_blocks] if isinstance(pag_blocks, str) else pag_blocks
        try:
            names = list(names)
        except TypeError:
            raise ValueError(f"pag_blocks must be a collection of names from {self.PAG_BLOCKS} "
                             f"(got {pag_blocks!r})") from None
        if not names or any(not isinstance(n, str) or n not in self.PAG_BLOCKS for n in names):
            raise ValueError(f"pag_blocks must be a non-empty collection of names from {self.PAG_BLOCKS} "
                             f"(got {pag_blocks!r})")
        if len(set(names)) != len(names):
            raise ValueError(f"pag_blocks names a block twice (got {pag_blocks!r})")
        blocks = sum(1 << self.PAG_BLOCKS.index(n) for n in names)
        if model is not None and _native_kind(model) not in (1, 2):
            if _native_kind(model) == 0:
                raise ValueError("pag_scale needs a dmx network: a foreign model's attention cannot be perturbed")
            raise ValueError("pag_scale needs a conditional model (UnetCond / UnetCondWithGeomHead)")
        try:
            phi = float(guidance_rescale)
        except (TypeError, ValueError):
            phi = float("nan")
        if guidance_interval is not None or phi != 0.0:
            raise ValueError("pag_scale takes no guidance_interval / guidance_rescale")
        if bool((self._weight_row(geom_scale, B, "geom_scale") != 0).any()):
            raise ValueError("pag_scale takes no geom_scale")
        s_row = row.to(device)
        if compose is not None:
            y_rows, v_rows, m_rows, w = compose
            if y_rows.shape[0] > self.COMPOSE_MAX:
                raise ValueError(f"pag_scale adds a branch: at most {self.COMPOSE_MAX - 2} specs in `also` with it "
                                 f"(got {y_rows.shape[0] - 2})")
            w = torch.cat([w[:1] + s_row, w[1:], -s_row[None]])
            y_rows, v_rows, m_rows = (torch.cat([r, r[1:2]]) for r in (y_rows, v_rows, m_rows))
        else:
            y_call = torch.tensor([int(c) for c in y_list], dtype=torch.long, device=device)
            v_call, m_call = vals.to(device).float(), msk.to(device).float()
            try:
                g = float(guidance_scale) if guidance_scale else 0.0
            except (TypeError, ValueError):
                raise ValueError(f"guidance_scale must be a number (got {guidance_scale!r})") from None
            if not np.isfinite(g):
                raise ValueError(f"guidance_scale must be finite (got {guidance_scale!r})")
            if g > 0:  # the plain CFG call as a composition, plus the perturbed branch
                ys = [torch.full_like(y_call, int(null_label)), y_call, y_call]
                w = torch.stack([torch.full((B,), g, dtype=torch.float32, device=device) + s_row, -s_row])
            else:      # no CFG: the main condition is the base
                ys = [y_call, y_call]
                w = -s_row[None]
            y_rows = torch.stack(ys)
            v_rows, m_rows = torch.stack([v_call] * len(ys)), torch.stack([m_call] * len(ys))
        K = y_rows.shape[0] - 1
        return (y_rows.contiguous(), v_rows.contiguous(), m_rows.contiguous(), w.contiguous()), (blocks, 1 << K)

    # ---- feature caching: the deep U-Net feature is refreshed every N-th step and reused between ----
    @staticmethod
    def _cache_args(cache_interval, model=None, composed=False, pag=False, geom=False, guidance_interval=None,
                    unguided_ddpm=False):
        """Argument rules of the samplers' cache_interval keyword -> N (1: the call without the keyword,
        which None and 1 both are).  N > 1 needs a dmx network and takes none of: composed guidance
        (`composed`: base / also / a per-sample guidance_scale), pag_scale (`pag`), geom_scale (`geom`), a
        guidance_interval (the rows of a step change between its segments), the ddpm sampler with
        guidance_scale 0 (`unguided_ddpm`: that loop mirrors the reference's unguided branch through the
        module's forward, which cannot be cut short).  Every violation raises
        ValueError naming both parties; nothing here touches the model or a GPU, and nothing is drawn."""
        if cache_interval is None:
            return 1
        if isinstance(cache_interval, bool) or not isinstance(cache_interval, int) or cache_interval < 1:
            raise ValueError(f"cache_interval must be None or an int >= 1 (got {cache_interval!r})")
        if cache_interval == 1:
            return 1
        if composed:
            raise ValueError("cache_interval takes no composed guidance (base / also / per-sample guidance_scale)")
        if pag:
            raise ValueError("cache_interval takes no pag_scale")
        if geom:
            raise ValueError("cache_interval takes no geom_scale")
        if guidance_interval is not None:
            raise ValueError("cache_interval takes no guidance_interval (the rows of a step change between segments)")
        if unguided_ddpm:
            raise ValueError('cache_interval with sampler="ddpm" needs guidance_scale > 0 (its unguided loop calls '
                             'the module\'s forward as the reference does); use a strided sampler for guidance_scale 0')
        if model is not None and _native_kind(model) == 0:
            raise ValueError("cache_interval needs a dmx network: a foreign model's forward cannot be cut short")
        return int(cache_interval)

    @staticmethod
    def _eps(model, x, t, y, null_label, cond_vals, cond_mask, g, rescale, compose):
        """A foreign model's prediction as the operands (eu, ec, g) of an update.  compose: one call per
        branch, then the mix (engine.compose_eps).  g > 0: the null-label and the conditional call, left
        to the update to mix or, with rescale = phi > 0, mixed and rescaled by the standalone kernel
        (engine.cfg_rescale).  Otherwise one call on y."""
        def eps_of(labels, v, m):
            e = model(x, t, labels, cond_vals=v, cond_mask=m)
            return e[0] if isinstance(e, (tuple, list)) else e

        if compose is not None:
            y_rows, v_rows, m_rows, w = compose
            es = [eps_of(y_rows[k].to(x.device), v_rows[k].to(x.device), m_rows[k].to(x.device))
                  for k in range(y_rows.shape[0])]
            return _engine.compose_eps(es, w), None, 0.0
        if g <= 0:
            return eps_of(y, cond_vals, cond_mask), None, 0.0
        eu, ec = eps_of(torch.full_like(y, null_label), cond_vals, cond_mask), eps_of(y, cond_vals, cond_mask)
        if rescale > 0:
            return _engine.cfg_rescale(eu, ec, g, float(rescale))[0], None, 0.0
        return eu, ec, g

    @staticmethod
    def _guided_run(tau, interval):
        """The positions of the ascending timesteps `tau` (tau_p at index p-1) whose step uses CFG:
        (p_lo, p_hi), inclusive, for the timesteps inside interval = (t_lo, t_hi); (1, S) for interval
        None; None when no timestep of the schedule lies inside.  tau ascends, so the run is contiguous."""
        S = len(tau)
        if interval is None:
            return (1, S)
        inside = [p for p in range(1, S + 1) if interval[0] <= tau[p - 1] <= interval[1]]
        return (inside[0], inside[-1]) if inside else None

    @staticmethod
    def _guidance_segments(i_from, i_to, run):
        """The steps at positions i_from, i_from - 1, .., i_to + 1 (a guard chunk, or a whole loop) cut
        where the step kind changes: a list of (a, b, guided), each covering positions a down to b + 1,
        guided iff they lie inside run = (p_lo, p_hi) (_guided_run; None: nothing is guided).  At most
        three segments, in walking order; empty when i_from <= i_to."""
        i_from, i_to = int(i_from), int(i_to)
        if i_from <= i_to:
            return []
        if run is None:
            return [(i_from, i_to, False)]
        p_lo, p_hi = run
        cuts = sorted({i_from, i_to, min(max(p_hi, i_to), i_from), min(max(p_lo - 1, i_to), i_from)}, reverse=True)
        return [(a, b, p_lo <= a <= p_hi) for a, b in zip(cuts, cuts[1:])]

    # ---- RNG -------------------------------------------------------------------------------
    _NOISE_RING = 3

    def _randn(self, shape, device):
        """One Gaussian draw in the reference's order (host mode) — diff.py:104,158,327.

        The draw is the global CPU generator's (torch.randn(shape, out=...) consumes it exactly like
        torch.randn(shape)).  For a GPU destination it lands in a small ring of pinned host buffers
        and goes up with a non-blocking copy, so the host draws step k+1's noise while the GPU runs
        step k (a pageable copy would block the host until the stream drained)."""
        shape = tuple(int(v) for v in shape)
        dev = torch.device(device)
        if dev.type != "cuda":
            return torch.randn(shape).to(dev)
        ring = self.__dict__.setdefault("_noise_ring", {})
        key = (shape, str(dev))
        slots = ring.get(key)
        if slots is None:
            slots = ring[key] = [[torch.empty(shape, pin_memory=True), None] for _ in range(self._NOISE_RING)]
            self.__dict__.setdefault("_noise_next", {})[key] = 0
        k = self._noise_next[key]
        self._noise_next[key] = (k + 1) % len(slots)
        buf, ev = slots[k]
        if ev is not None:
            ev.synchronize()  # the copy that last read this pinned slot has finished
        torch.randn(shape, out=buf)
        out = buf.to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        slots[k][1] = ev
        return out

    def _step_noise(self, x):
        if self.noise_source == "host":
            pf = self.__dict__.get("_prefetch")
            if pf is not None and x.is_cuda and tuple(x.shape) == pf.shape:
                return pf.next(x.device)
            return self._randn(x.shape, x.device)
        return None

    def _seed(self) -> int:
        return int(torch.randint(0, 2 ** 62, (1,)).item())

    # ---- training-side helper (not on the sampling path) ------------------------------------
    def add_noise(self, x_0, t):
        """diff.py:18-30 — forward diffusion used by training (plain torch; not a dmx path)."""
        assert (t >= 1).all() and (t <= self.num_timesteps).all()
        ab = self.alpha_bars[t - 1].view(-1, 1, 1, 1)
        noise = torch.randn_like(x_0, device=self.device)
        return torch.sqrt(ab) * x_0 + torch.sqrt(1 - ab) * noise, noise

    # ---- the training objective (no reference counterpart as one call: train_latent_cond.py:136-162) ----
    def noise_tables(self, device):
        """(sa, s1) = sqrt(ab), sqrt(1 - ab) per t-1: add_noise's two coefficients, evaluated by torch on
        `device` (the bits add_noise gets there)."""
        key = ("noise", str(device))
        if key not in self._tables:
            ab = self._host[1].to(device)
            self._tables[key] = (torch.sqrt(ab).contiguous(), torch.sqrt(1 - ab).contiguous())
        return self._tables[key]

    def loss_weights(self, weighting="uniform", snr_gamma=5.0, device=None):
        """Per-timestep weights of the noise loss, (T,) fp32, index t-1.  "uniform": ones (the reference's
        F.mse_loss).  "min_snr": min(SNR_t, gamma) / SNR_t with SNR_t = ab_t / (1 - ab_t), the
        eps-prediction form of min-SNR-gamma (Hang et al. 2023, "Efficient diffusion training via min-SNR
        weighting strategy"), evaluated in float64 and rounded once.  A v-model (prediction="v") takes the
        paper's v-prediction form min(SNR_t, gamma) / (SNR_t + 1), formed the same way; it is finite everywhere
        and 0 at t = T of a zero-terminal-SNR schedule (SNR_T = 0): the pure-noise step then carries no weight."""
        try:
            gamma = float(snr_gamma)
        except (TypeError, ValueError):
            gamma = float("nan")
        if isinstance(snr_gamma, (bool, str)) or not (gamma > 0.0 and math.isfinite(gamma)):
            raise ValueError(f"snr_gamma must be a positive finite number (got {snr_gamma!r})")
        if weighting not in ("uniform", "min_snr"):
            raise ValueError(f'weighting must be "uniform" or "min_snr" (got {weighting!r})')
        device = self.device if device is None else device
        key = ("weights", weighting, gamma, str(device), self.prediction)
        if key not in self._tables:
            if weighting == "uniform":
                w = torch.ones(self.num_timesteps, dtype=torch.float32)
            else:
                ab = self._host[1].double()
                snr = ab / (1 - ab)
                w = (torch.clamp(snr, max=gamma) / (snr + 1 if self.prediction == "v" else snr)).float()
            self._tables[key] = w.contiguous().to(device)
        return self._tables[key]

    def training_loss(self, model, z, classes, cond=None, cond_mask=None, *, geom_lambda=0.0, cfg_drop_prob=0.0,
                      null_label=0, weighting="uniform", snr_gamma=5.0, t=None, noise=None, drop=None,
                      geom_denom=None, sample_offset=0):
        """One training iteration's objective on the latents z (B,C,h,w) with labels `classes` (B,) and the
        numeric condition cond / cond_mask (B,gd) -> TrainingLoss.  What train_latent_cond.py:136-159 spells
        out in torch ops:
            t ~ U{1..T};  z_noisy = sqrt(ab_t) z + sqrt(1 - ab_t) noise;  drop ~ (u < cfg_drop_prob)
            y_used = where(drop, null_label, classes);  vals_used, mask_used = cond, cond_mask zeroed where drop
            eps, geom = model(z_noisy, t, y_used, cond_vals=vals_used, cond_mask=mask_used)
            per_sample[n] = w[t_n] mean_chw (eps - target)^2;  noise_loss = mean_n per_sample[n]
            target = noise, or for a v-model (prediction="v") sqrt(ab_t) noise - sqrt(1 - ab_t) z
            geom_loss = sum mask_used (geom - cond)^2 / max(denom, 1e-6)   (denom = sum mask_used unless geom_denom)
            loss = noise_loss + geom_lambda geom_loss
        with w = loss_weights(weighting, snr_gamma): "uniform" is the reference's loss.  t, noise and drop
        given are used as they are (t is range-checked, which reads it back); each one omitted is drawn.

        A dmx U-Net on the GPU: the draws are Philox's on the device under one seed taken from torch's
        global generator (torch.manual_seed fixes the batch), addressed by the rows' global indices
        sample_offset + n, so a data-parallel rank with sample_offset = rank * B draws its rows of the
        global batch; the objective runs in the native kernels (dmx_train_noise / dmx_objective_loss), and in
        training mode with autograd recording `loss` is one autograd node over the parameters whose backward
        seeds the native backward on the device (dmx_objective_seed): loss.backward(), (loss / k).backward()
        and loss * scale work without a host synchronisation, and with drawn t the call itself issues
        none.  In eval mode or under no_grad the same kernels run around the ordinary forward, no tape.
        Any other model (or device): the same definition in torch ops, draws from torch's generators on z's
        device (sample_offset is not used), autograd for the backward."""
        T = int(self.num_timesteps)
        if weighting not in ("uniform", "min_snr"):
            raise ValueError(f'weighting must be "uniform" or "min_snr" (got {weighting!r})')
        if z.dim() != 4 or min(z.shape) < 1:
            raise ValueError(f"z must be a non-empty (B,C,h,w) tensor (got {tuple(z.shape)})")
        B = int(z.shape[0])
        if classes.dim() != 1 or classes.shape[0] != B:
            raise ValueError(f"classes must be ({B},) (got {tuple(classes.shape)})")
        if (cond is None) != (cond_mask is None):
            raise ValueError("cond and cond_mask go together")
        if cond is not None and (cond.dim() != 2 or cond.shape[0] != B or cond.shape[1] < 1
                                 or tuple(cond_mask.shape) != tuple(cond.shape)):
            raise ValueError(f"cond / cond_mask must be equal ({B}, gd) tensors (got {tuple(cond.shape)}, "
                             f"{tuple(cond_mask.shape)})")
        for v, nm, shape in ((t, "t", (B,)), (noise, "noise", tuple(z.shape)), (drop, "drop", (B,))):
            if v is not None and tuple(v.shape) != shape:
                raise ValueError(f"{nm} must be {shape} (got {tuple(v.shape)})")
        lam, p = float(geom_lambda), float(cfg_drop_prob)
        if not (lam >= 0.0 and math.isfinite(lam)):
            raise ValueError(f"geom_lambda must be finite and >= 0 (got {geom_lambda})")
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"cfg_drop_prob must be in [0, 1] (got {cfg_drop_prob})")
        if drop is not None and p != 0.0:
            raise ValueError("drop is given: cfg_drop_prob must be 0")
        kind = _native_kind(model)
        has_head = kind == 1 if kind else getattr(model, "geom_head", None) is not None
        if lam != 0.0 and (not has_head or cond is None):
            raise ValueError("geom_lambda != 0 needs a model with a GeomHead and cond / cond_mask (its target)")
        if kind == 2 and model.training and float(model.cfg_drop_prob) > 0.0:
            raise ValueError("UnetCond draws a dropout of its own in forward (cfg_drop_prob > 0): construct it with "
                             "cfg_drop_prob=0 and give the probability to training_loss")
        weights = self.loss_weights(weighting, snr_gamma, z.device)
        if t is not None and not bool(((t >= 1) & (t <= T)).all()):
            raise ValueError(f"t must lie in [1, {T}]")
        if geom_denom is not None:
            geom_denom = torch.as_tensor(geom_denom, dtype=torch.float32).to(z.device)
        if kind in (1, 2) and z.is_cuda:
            return self._training_loss_native(model, z, classes, cond, cond_mask, lam, p, null_label,
                                              None if weighting == "uniform" else weights, t, noise, drop,
                                              geom_denom, sample_offset)
        dev = z.device
        if t is None:
            t = torch.randint(1, T + 1, (B,), device=dev)
        if noise is None:
            noise = torch.randn_like(z)
        if drop is None:
            drop = torch.rand(B, device=dev) < p
        t, drop = t.to(dev), drop.to(device=dev, dtype=torch.bool)
        ab = self._host[1].to(dev)[t - 1].view(-1, 1, 1, 1)
        z_noisy = torch.sqrt(ab) * z + torch.sqrt(1 - ab) * noise
        y_used = torch.where(drop, torch.full_like(classes, null_label), classes)
        if cond is not None:
            keep = (~drop).float().unsqueeze(1)
            vals_used, mask_used = cond * keep, cond_mask * keep
            out = model(z_noisy, t, y_used, cond_vals=vals_used, cond_mask=mask_used)
        else:
            out = model(z_noisy, t, y_used)
        eps, geom = out if isinstance(out, tuple) else (out, None)
        target = noise if self.prediction != "v" else torch.sqrt(ab) * noise - torch.sqrt(1 - ab) * z
        per_sample = weights[t - 1] * (eps - target).pow(2).flatten(1).mean(dim=1)
        noise_loss = per_sample.mean()
        geom_loss = torch.zeros((), device=dev)
        if geom is not None and cond is not None:
            from losses.geom_losses import masked_geom_mse
            geom_loss = masked_geom_mse(geom, cond, mask_used, denom=geom_denom)
        loss = noise_loss + lam * geom_loss
        return TrainingLoss(loss, noise_loss.detach(), geom_loss.detach(), per_sample.detach(), t, drop,
                            eps.detach(), geom.detach() if geom is not None else None, target.detach())

    def _training_loss_native(self, model, z, classes, cond, cond_mask, lam, p, null_label, weights, t, noise, drop,
                              geom_denom, sample_offset):
        """training_loss on a dmx conditional U-Net on the GPU (arguments checked there)."""
        from models._native import _NativeObjectiveFn
        T = int(self.num_timesteps)
        sa, s1 = self.noise_tables(z.device)
        seed = self._seed() if (t is None or noise is None or drop is None) else 0
        # a v-model: the noising launch also stores the target, and the loss kernels read it where they read noise
        front = _engine.train_noise(z, sa, s1, t, noise, drop, classes, null_label, cond, cond_mask, p, seed,
                                    sample_offset, **({"target": True} if self.prediction == "v" else {}))
        z_noisy, noise, t, drop, y_used, vals_used, mask_used = front[:7]
        target = front[7] if self.prediction == "v" else noise
        if model.training and model._dmx_training():
            bad = [n for n, q in model.named_parameters() if q.dtype != torch.float32 or not q.is_contiguous()]
            if bad:
                raise NotImplementedError(f"dmx training needs contiguous fp32 parameters ({bad[0]})")
            # t lies in [1, T] (drawn so, or checked by training_loss): train_forward need not read it back
            job = dict(z_noisy=z_noisy, t=t, y=y_used, vals_used=vals_used, mask_used=mask_used, noise=target,
                       vals=cond, weight=weights, geom_lambda=lam, denom=geom_denom, tmax=T)
            names = [n for n, _ in model.named_parameters()]
            loss, out, per_sample, eps, geom = _NativeObjectiveFn.apply(model, names, job, *model.parameters())
            geom = geom if geom.numel() else None
        else:
            with torch.no_grad():
                res = (model(z_noisy, t, y_used, cond_vals=vals_used, cond_mask=mask_used) if cond is not None
                       else model(z_noisy, t, y_used))
                eps, geom = res if isinstance(res, tuple) else (res, None)
                use_geom = geom is not None and cond is not None
                obj = _engine.objective_loss(eps, target, t, weights, geom if use_geom else None,
                                             cond if use_geom else None, mask_used if use_geom else None, lam,
                                             geom_denom)
            loss, out, per_sample = obj.loss, obj._out, obj.per_sample
        return TrainingLoss(loss, out[1], out[2], per_sample, t, drop, eps, geom, target)

    # ---- one step -----------------------------------------------------------------------------
    def denoise(self, model, x, t):
        """Unconditional DDPM step (diff.py:32-56)."""
        T = self.num_timesteps
        assert (t >= 1).all() and (t <= T).all()
        # (the x0-form takes alpha_bar_prev = 1 at t = 1 here too: the wrap-around is an eps-mode parity quirk)
        tables = self.coef_tables(x.device, clamp_prev=self.x0_form)
        model.eval()
        if _native_kind(model) and x.is_cuda and getattr(model, "_dmx_kind", 0) == 3:
            model.train()
            noise = self._step_noise(x)
            out = torch.empty_like(x)
            self._native(model).step(x, out, t.to(x.device), None, 0, None, None, 0.0, tables, noise,
                                     seed=self._seed() if noise is None else 0)
            return out
        with torch.no_grad():
            eps = self._to_eps(model(x, t), None, 0.0, x, t)[0]
        model.train()
        noise = self._step_noise(x)
        return _engine.ddpm_update(x, eps, None, 0.0, t, tables, noise, seed=self._seed() if noise is None else 0)

    def reverse_to_img(self, x):
        """diff.py:58-64: x*255 -> clamp(0,255) -> uint8 (truncation) -> PIL."""
        from PIL import Image
        a = (x * 255).clamp(0, 255).to(torch.uint8).cpu().numpy()
        if a.ndim == 3:
            a = np.transpose(a, (1, 2, 0))
            if a.shape[2] == 1:
                a = a[:, :, 0]
        return Image.fromarray(a)

    def denoise_cond(self, model, x, t, y=None, guidance_scale=0.0, null_label=0, cond_vals=None, cond_mask=None):
        """One DDPM step with optional classifier-free guidance (diff.py:127-162)."""
        T = self.num_timesteps
        assert (t >= 1).all() and (t <= T).all()  # (reads t back: a device sync, as in the reference)
        plan = _SamplerPlan("ddpm", tables=self.coef_tables(x.device, clamp_prev=True),
                            scale=float(guidance_scale) if guidance_scale else 0.0)
        return self._step(model, x, t, plan, True, y, null_label, cond_vals, cond_mask)

    def _step(self, model, x, pos, plan, guided, y=None, null_label=0, cond_vals=None, cond_mask=None, hist=None,
              phase=0):
        """One step of plan.rule at `pos` ((B,): timesteps for ddpm, positions of plan.sched otherwise —
        countdown rows of an inversion, whose `hist` is its source latent)
        after the public entries' range checks — the samplers' loops build pos from a host-known
        counter and call this directly, so the host never waits on the device per step.
        guided: CFG (plan.scale > 0 and y given; rescaled for plan.rescale > 0), else one conditional
        forward (the steps outside a guidance interval; y defaults to null_label on the strided
        rules).  A ddpm step that asks for guidance but cannot have it is the reference's plain branch,
        mirrored literally.  plan.compose: the composed step, which reads none of y, vals, mask.
        A dmx network on the GPU runs it as one native step, known-region blend included; any other
        model is called like the reference and the update and the blend run natively after it.
        The native step draws its noise (host mode) or seed (device mode) before the step, the
        foreign one after the model's forwards; a rule that draws nothing consumes neither.
        phase: the step's offset in its guard chunk, which decides whether a cached plan's step refreshes
        the feature or reuses it; only the native step can do either."""
        rule, compose = plan.rule, plan.compose
        g = plan.scale if guided and compose is None and y is not None and plan.scale > 0 else 0.0
        mirror = rule == "ddpm" and guided and compose is None and g == 0.0
        if rule != "ddpm":
            pos = pos.to(device=x.device, dtype=torch.long)
            if y is None and compose is None:
                y = torch.full((x.size(0),), null_label, device=x.device, dtype=torch.long)

        def draw():  # -> (noise, seed): host noise, else a seed where the rule draws at all
            noise = self._step_noise(x) if plan.draws else None
            return noise, self._seed() if plan.draws and noise is None else None

        with torch.no_grad():
            if _native_kind(model) in (1, 2) and x.is_cuda and not mirror:
                noise, seed = draw()
                x_in = x.contiguous() if rule == "ddpm" else x.float().contiguous()
                out = torch.empty_like(x_in)
                use = cond_vals is not None and cond_mask is not None
                nm = self._native(model)
                nm.step(x_in, out, pos.to(x.device), None if y is None else y.to(x.device), null_label,
                        cond_vals if use else None, cond_mask if use else None, g, plan.tables, noise,
                        **plan.kwargs(g > 0, hist, seed=seed, phase=phase))
                return out
            if plan.cache > 1:
                raise ValueError("cache_interval needs a dmx network on the GPU: only the native step can reuse "
                                 "the cached feature")
            if plan.perturb is not None:
                raise ValueError("pag_scale needs a dmx network on the GPU: only the native step can perturb attention")
            t = pos if rule == "ddpm" else plan.sched[0][pos - 1]
            if not mirror:
                eu, ec, g = self._eps(model, x, t, y, null_label, cond_vals, cond_mask, g, plan.rescale, compose)
                if plan.geom is not None and ec is not None:  # the guided eps, then the gradient's share
                    grad = self._geom_loss_grad(model, x, t, y, cond_vals, cond_mask)
                    eu, ec, g = _engine.geom_mix(eu + g * (ec - eu), grad, plan.geom[0], plan.geom[1], pos), None, 0.0
                eu, ec, g = self._to_eps(eu, ec, g, x, t)
            elif y is None:  # diff.py:152-156 literally, including its UnboundLocalError when y is given
                y = torch.full((x.size(0),), null_label, device=x.device, dtype=torch.long)
                eu, ec = model(x, t, y, cond_vals=cond_vals, cond_mask=cond_mask), None
        noise, seed = draw()
        if mirror and not isinstance(eu, torch.Tensor):
            raise TypeError(f"unsupported operand type(s) for *: 'Tensor' and '{type(eu).__name__}'")
        if mirror:
            eu, ec, g = self._to_eps(eu, ec, g, x, t)
        if rule == "ddpm":
            out = _engine.ddpm_update(x, eu, ec, g, pos, plan.tables, noise, seed=seed or 0)
        elif rule == "ddim":
            out = _engine.ddim_update(x, eu, ec, g, pos, plan.sched, noise, seed=seed or 0)
        elif rule == "invert":
            out = _engine.invert_update(x, eu, ec, g, pos, plan.sched, hist)
        else:
            out = _engine.dpm_update(x, eu, ec, g, pos, plan.sched, hist)
        return self._blend(out, pos, plan.known)

    @staticmethod
    def _blend(x, pos, known):
        """The known-region blend after a foreign model's update, in place on the update's output."""
        return x if known is None else _engine.known_blend(x, pos, known, out=x)

    def ddim_step(self, model, x, pos, steps, eta=0.0, y=None, guidance_scale=0.0, null_label=0, cond_vals=None,
                  cond_mask=None):
        """One strided DDIM step at position(s) `pos` ((B,) in [1, steps]) of the `steps`-position
        schedule: from timestep tau_pos to tau_{pos-1} (ddim_tables).  CFG when guidance_scale > 0 and y
        is given, otherwise one conditional forward (y defaults to null_label)."""
        S = len(self.ddim_timesteps(steps))
        assert (pos >= 1).all() and (pos <= S).all()  # (reads pos back: a device sync, as denoise_cond)
        plan = _SamplerPlan("ddim", sched=self.ddim_tables(steps, eta, x.device), draws=float(eta) > 0,
                            scale=float(guidance_scale) if guidance_scale else 0.0)
        return self._step(model, x, pos, plan, True, y, null_label, cond_vals, cond_mask)

    def dpm_step(self, model, x, pos, hist, steps, spacing="logsnr", y=None, guidance_scale=0.0, null_label=0,
                 cond_vals=None, cond_mask=None):
        """One DPM-Solver++(2M) step at position(s) `pos` ((B,) in [1, steps]) of the `steps`-position
        schedule of dpm_tables(steps, spacing): returns x' and leaves this step's x0 in `hist` (fp32,
        x's shape, updated in place).  Below position `steps`, hist must hold the x0 that the step at
        pos + 1 left; positions `steps` and 1 do not read it.  Draws nothing.  CFG as in ddim_step."""
        S = len(self.dpm_timesteps(steps, spacing))
        assert (pos >= 1).all() and (pos <= S).all()  # (reads pos back: a device sync, as denoise_cond)
        plan = _SamplerPlan("dpm", sched=self.dpm_tables(steps, spacing, x.device), draws=False,
                            scale=float(guidance_scale) if guidance_scale else 0.0)
        return self._step(model, x, pos, plan, True, y, null_label, cond_vals, cond_mask, hist)

    # ---- loops --------------------------------------------------------------------------------
    def sample(self, model, x_shape=(20, 3, 80, 80)):
        """Pixel-space sampler (diff.py:66-85)."""
        batch_size = x_shape[0]
        x = self._randn(x_shape, self.device)
        for i in tqdm(range(self.num_timesteps, 0, -1)):
            t = torch.tensor([i] * batch_size, device=self.device, dtype=torch.long)
            x = self.denoise(model, x, t)
        return [self.reverse_to_img(x[i]) for i in range(batch_size)]

    def sample_latent(self, model, z_shape=(1000, 4, 28, 28), vae=None, to_pil=True, progress=True):
        """Latent sampler, unconditional model (diff.py:87-125)."""
        batch_size = z_shape[0]
        x = self._randn(z_shape, self.device)
        bar = tqdm(total=self.num_timesteps) if progress else None

        def run(i_from, i_to, x):
            for i in range(i_from, i_to, -1):
                t = torch.full((batch_size,), i, device=self.device, dtype=torch.long)
                x = self.denoise(model, x, t)
                if bar is not None:
                    bar.update(1)
            return x

        with torch.no_grad():
            x = self._guarded_loop(self._prefetching(run, model, x), x, self.num_timesteps,
                                   self._guard_target(model, x))
        if bar is not None:
            bar.close()
        if vae is None:
            return x
        return self._decode(vae, x, to_pil)

    # ---- split-precision range guard ------------------------------------------------------
    GUARD_CHUNK = 50

    @staticmethod
    def _guard_target(model, x=None):
        """The NativeModel whose range flag guards this loop (None: foreign model, exact fp32, or a
        loop on the host tensor x)."""
        if not _native_kind(model) or (x is not None and not x.is_cuda):
            return None
        nm = model.native()
        return nm if nm.precision != "fp32" else None

    def _guarded_loop(self, run, x, start, guard, hist=None, inplace=False, on_replay=None, any_rank=None,
                      owner=None):
        """The positions start .. 1 in chunks of GUARD_CHUNK; `run(i_from, i_to, x)` advances
        i_from .. i_to + 1 and returns x, which it steps in place (`inplace`: the device loop) or
        replaces.  After each chunk the range flag of `guard` (a NativeModel, or None) is read
        (dmx_model_range_check) and combined over the ranks by `any_rank` where given; if an operand
        left the f16 range of the split-precision modes the chunk is replayed from its start — same
        x, same solver history `hist`, same CPU-generator state, hence the same draws — in exact-fp32
        MFMA mode (a rank without a guard just reruns it), after `on_replay()`, and `owner`
        (default: this Diffuser) counts one range_fallbacks.  The chunk's start is kept only where a
        replay can happen; an in-place runner needs a copy of it."""
        keep = guard is not None or any_rank is not None
        i = int(start)
        while i >= 1:
            j = max(i - self.GUARD_CHUNK, 0)
            if keep:
                x0, rng = x.clone() if inplace else x, torch.get_rng_state()
                h0 = hist.clone() if hist is not None else None
            x = run(i, j, x)
            tripped = guard is not None and guard.range_tripped()
            if any_rank(tripped) if any_rank is not None else tripped:
                if on_replay is not None:
                    on_replay()
                torch.set_rng_state(rng)
                x = x.copy_(x0) if inplace else x0
                if hist is not None:
                    hist.copy_(h0)
                with guard.precision_override("fp32") if guard is not None else contextlib.nullcontext():
                    x = run(i, j, x)
                if guard is not None:
                    guard.range_tripped()  # clear
                owner = self if owner is None else owner
                owner.range_fallbacks += 1
            i = j
        return x

    def _prefetching(self, run, model, x, draws=True):
        """`run` with each chunk's host-noise draws made ahead on a helper thread (_NoisePrefetch),
        where the chunk's steps draw host noise for a dmx network on the GPU; else `run` itself."""
        if not (draws and x.is_cuda and self.noise_source == "host" and _native_kind(model) != 0):
            return run

        def chunk(i, j, x):
            self._prefetch = _NoisePrefetch(x.shape, i - j)
            try:
                return run(i, j, x)
            finally:
                pf, self._prefetch = self._prefetch, None
                pf.close()
        return chunk

    def sample_cond(self, model, x_shape, y, guidance_scale=0.0, null_label=0):
        """diff.py:165-172."""
        batch_size = x_shape[0]
        assert y.shape[0] == batch_size
        x = self._randn(x_shape, self.device)
        for i in range(self.num_timesteps, 0, -1):
            t = torch.full((batch_size,), i, device=self.device, dtype=torch.long)
            x = self.denoise_cond(model, x, t, y=y, guidance_scale=guidance_scale, null_label=null_label)
        return x

    def _decode(self, vae, x, to_pil):
        """Decode latents; dmx VAEs emit the uint8 HWC images directly (diff.py:346-369)."""
        if _native_kind(vae) == 4 and x.is_cuda:
            img, u8 = vae.native().decode(x, want_img=not to_pil, want_u8=to_pil)
            if to_pil:
                from PIL import Image
                arr = u8.cpu().numpy()
                return [Image.fromarray(arr[i]) for i in range(arr.shape[0])]
            return img
        vae.eval()
        outs = []
        with torch.inference_mode():
            for s in range(0, x.shape[0], 4):
                outs.append(vae.decode(x[s:s + 4]))
        images = torch.cat(outs, dim=0)
        return [self.reverse_to_img(images[i]) for i in range(images.shape[0])] if to_pil else images

    @staticmethod
    def _norm_counts(cc) -> List[Tuple[int, int]]:
        """diff.py:206-218."""
        if isinstance(cc, dict):
            items = list(cc.items())
        elif isinstance(cc, tuple) and len(cc) == 2:
            items = [cc]
        elif isinstance(cc, list):
            items = list(cc)
        else:
            raise ValueError("class_counts は {cls:num}, (cls,num), そのリストのいずれか。")
        items = [(int(c), int(n)) for c, n in items if int(n) > 0]
        if not items:
            raise ValueError("生成枚数が0です。")
        return items

    def _build_cond(self, y_list, cond, cond_mask, key_order, class_keys, device):
        """(B,K) vals/mask from tensor / dict / list inputs (diff.py:229-312)."""
        B = len(y_list)
        if key_order is None:
            key_order = list(KEY_ORDER)
        K = len(key_order)
        kidx = {k: i for i, k in enumerate(key_order)}
        if class_keys is None:
            class_keys = CLASS_KEYS
        vals = cond.to(device) if isinstance(cond, torch.Tensor) else None
        msk = cond_mask.to(device) if isinstance(cond_mask, torch.Tensor) else None
        if vals is not None:
            if vals.ndim != 2 or vals.shape[0] != B or vals.shape[1] != K:
                raise ValueError(f"cond Tensor 形状は (B={B}, K={K}) 必須: got {tuple(vals.shape)}")
            if msk is None:
                msk = (vals != 0).float()
            elif msk.ndim != 2 or msk.shape != vals.shape:
                raise ValueError("cond_mask Tensor 形状は cond と同じ (B,K) 必須。")
            return vals, msk
        vals = torch.zeros((B, K), device=device, dtype=torch.float32)
        if msk is None:
            msk = torch.zeros((B, K), device=device, dtype=torch.float32)
        if isinstance(cond, dict):
            for i, cls in enumerate(y_list):
                if cls in cond:
                    for k, v in cond[cls].items():
                        if k not in kidx:
                            continue
                        vals[i, kidx[k]] = float(v)
                        explicit = isinstance(cond_mask, dict) and cls in cond_mask and k in cond_mask[cls]
                        msk[i, kidx[k]] = float(cond_mask[cls][k]) if explicit else 1.0
                if isinstance(cond_mask, dict) and cls in cond_mask:
                    for k, mv in cond_mask[cls].items():
                        if k in kidx:
                            msk[i, kidx[k]] = float(mv)
        elif isinstance(cond, list):
            if len(cond) != B:
                raise ValueError(f"cond(list) の長さ {len(cond)} が生成枚数 {B} と不一致。")
            for i, d in enumerate(cond):
                for k, v in d.items():
                    if k not in kidx:
                        continue
                    vals[i, kidx[k]] = float(v)
                    explicit = isinstance(cond_mask, list) and i < len(cond_mask) and k in cond_mask[i]
                    msk[i, kidx[k]] = float(cond_mask[i][k]) if explicit else 1.0
            if isinstance(cond_mask, list) and len(cond_mask) == B:
                for i, d in enumerate(cond_mask):
                    for k, mv in d.items():
                        if k in kidx:
                            msk[i, kidx[k]] = float(mv)
        else:
            for i, cls in enumerate(y_list):
                for k in class_keys.get(cls, []):
                    if k in kidx:
                        msk[i, kidx[k]] = 1.0
        return vals, msk

    def _latent_shape(self, vae, dummy_input_hw, device):
        """z_shape inference (diff.py:315-322).  For a dmx VAE the encoder is not run:
        the shape follows from its conv arithmetic and its randn_like draw
        (models/vae.py:56) is replayed so the global RNG stream stays aligned."""
        H, W = dummy_input_hw
        if _native_kind(vae) == 4:
            from models.vae import latent_hw
            h, w = latent_hw(H, W)
            if self.noise_source == "host":
                torch.randn((1, vae.z_channels, h, w))
            return vae.z_channels, h, w
        with torch.no_grad():
            z, _ = vae.encode(torch.zeros(1, 3, H, W, device=device))
        return tuple(z.shape[1:])

    def sample_latent_cond(
        self,
        model,
        class_counts: Union[Dict[int, int], Tuple[int, int], List[Tuple[int, int]]],
        z_shape: Tuple[int, int, int] = None,
        vae=None,
        to_pil: bool = True,
        progress: bool = True,
        guidance_scale: float = 3.0,
        null_label: int = 0,
        dummy_input_hw: Tuple[int, int] = (224, 224),
        cond=None,
        cond_mask=None,
        key_order: Optional[List[str]] = None,
        class_keys: Optional[Dict[int, List[str]]] = None,
        sampler: str = "ddpm",
        steps: Optional[int] = None,
        eta: float = 0.0,
        spacing: Optional[str] = None,
        init_latent: Optional[torch.Tensor] = None,
        mask: Optional[torch.Tensor] = None,
        strength: Optional[float] = None,
        guidance_interval: Optional[Tuple[int, int]] = None,
        guidance_rescale: float = 0.0,
        base="null",
        also=None,
        geom_scale=0.0,
        pag_scale=0.0,
        pag_blocks=("sa3",),
        start_latent: Optional[torch.Tensor] = None,
        cache_interval: Optional[int] = None,
    ):
        """Class + numeric-condition latent sampler (diff.py:174-369).

        sampler="ddim", steps=S (1 <= S <= num_timesteps), eta in [0, 1]: S strided DDIM steps over
        ddim_timesteps(S) instead of all T (eta = 0 deterministic, eta = 1 strided ancestral sampling).
        Draw order in host-noise mode with eta > 0 is the DDPM sampler's (optional encode draw, x_T, one
        global draw per step); eta = 0 draws nothing after x_T.

        sampler="dpmpp_2m", steps=S, spacing=None / "logsnr" (the default) or "uniform": S steps of
        DPM-Solver++(2M) over dpm_timesteps(S, spacing).  Deterministic (eta must be 0): only x_T is
        drawn.  `spacing` belongs to this sampler alone.

        init_latent = z0 ((B,C,h,w), (1,C,h,w) or (C,h,w), broadcast to the batch; e.g. vae.encode(img)[0]),
        with any sampler: image-conditioned sampling.  The one draw made for x_T, at its usual place in
        the draw order, is the fixed noise e0 of the call.
        strength in (0, 1]: img2img — the loop enters at position p0 = min(S, max(1, floor(strength S + 0.5)))
        of its S positions (T for ddpm) from sqrt(ab) z0 + sqrt(1 - ab) e0 at that position's timestep
        and runs p0 steps; None or p0 = S starts from e0 as every call does.
        mask ((B,1,h,w), (1,1,h,w) or (h,w) in [0, 1]; 1 = regenerate, 0 = keep): inpainting — after
        every step the latent is blended with z0's forward trajectory under e0 (known_tables), so the
        result equals z0 exactly where mask == 0.  mask / strength need init_latent; with z_shape None
        the shape is init_latent's and the VAE is not consulted (no encode draw).

        guidance_interval = (t_lo, t_hi), network timesteps with 1 <= t_lo <= t_hi <= num_timesteps, with
        any sampler (Kynkäänniemi et al. 2024): a step whose timestep lies inside uses CFG, every other
        step takes the conditional prediction alone — one B-sample forward instead of the 2B one.  An
        interval that holds no timestep of the schedule leaves the whole loop conditional-only; None
        guides every step.  guidance_rescale = phi in [0, 1] (Lin et al. 2023, §3.4), guided steps only:
        the guided prediction eg is scaled per sample by 1 + phi (std(ec) / std(eg) - 1), ec being the
        conditional prediction.  Both need guidance_scale > 0 and neither changes the draw order.

        Composed guidance (Liu et al. 2022), with any sampler, init_latent and mask:
        eps = e_0 + sum_k w_k (e_k - e_0) over a base branch 0 and up to four condition branches, run as
        one (K+1) B forward per step.  base = "null" (the default): null label with the call's cond /
        cond_mask, the reference's unconditional branch; "dropped": null label with cond = cond_mask = 0,
        the input training's joint condition dropout produced; a condition spec: a negative condition to
        steer away from.  The call's own condition is branch 1 with weight guidance_scale, which may be
        B finite floats (a per-sample guidance scale); also = up to three condition specs, each a dict
        {"classes": int or B ints, "cond": .., "cond_mask": .. (every form `cond` takes), "weight": float
        or B floats}.  With base "null", no `also` and a scalar guidance_scale the call is the plain one.
        A composed call takes no guidance_interval / guidance_rescale; the draw order is unchanged.

        geom_scale = s (a float or B finite floats, >= 0; UnetCondWithGeomHead, or a foreign model whose
        forward returns (eps, geom)), with any sampler, init_latent and mask: geometry guidance
        (classifier guidance, Dhariwal & Nichol 2021 §4.1).  Every step adds s sqrt(1 - ab_t) dL/dx_t
        to its CFG-guided prediction, L the GeomHead's masked squared error against the call's own
        cond / cond_mask per sample — it pulls the sample towards the numbers it is conditioned on.  A
        step then costs the CFG forward plus a taped forward and a data-only backward of B rows.  It
        needs a scalar guidance_scale > 0 and `cond`, and takes no guidance_interval, guidance_rescale,
        base or also; a row whose mask is all zero is not guided.  0 (the default) is the call without
        the keyword; the draw order is unchanged.

        pag_scale = s (a float or B finite floats, >= 0; a conditional dmx network), with any sampler,
        init_latent, mask, base and also: perturbed-attention guidance (Ahn et al. 2024).  Every step runs one
        more branch — the call's own condition again, with the self-attention of the blocks in pag_blocks
        (names from "sa1".."sa6"; "sa1".."sa3" the down path, "sa4".."sa6" the up path) replaced by the
        identity — and pushes the prediction away from it: eps = e_u + g (e_c - e_u) + s (e_c - e_p).
        It acts where CFG has nothing to act on: with guidance_scale 0 the step is e_c + s (e_c - e_p),
        at the cost of a CFG step.  At most two specs in `also` with it; no guidance_interval,
        guidance_rescale or geom_scale.  0 (the default) is the call without the keywords; the draw
        order is unchanged.

        start_latent = x ((B,C,h,w), (1,C,h,w) or (C,h,w), broadcast to the batch), with sampler="ddim" or
        "dpmpp_2m": the loop starts from x as it is — no noise is added to it — at position
        p0 = min(S, max(1, floor(strength S + 0.5))) (S for strength None) and runs p0 steps.  With
        x = invert_latent_cond(..., steps=S, strength=strength) and eta = 0 this is the way back from an
        inverted latent, under the same or an edited condition.  It excludes init_latent and mask;
        z_shape defaults to x's shape.  Draw order: no x_T draw is made and, with z_shape None, no encode
        draw either; ddim with eta > 0 still draws once per step, everything else draws nothing.
        Without the keyword the call is what it is today, `strength` without init_latent an error.

        cache_interval = N (an int >= 1; a dmx network), with any sampler, guidance_rescale, init_latent / mask /
        strength and start_latent: feature caching (DeepCache, Ma et al. 2024).  Every N-th step runs the whole
        network and keeps its deepest up-path feature (sa5's output); the N - 1 steps between run only inc,
        up3, sa6 and the head on the kept feature.  The count restarts with every guard chunk (GUARD_CHUNK
        positions), so each chunk begins with a full step.  An approximation, off by default: None and 1 are the
        call without the keyword.  It takes no composed guidance, pag_scale, geom_scale or guidance_interval,
        and the draw order is unchanged."""
        mode = self._sampler_mode(sampler, steps, eta, spacing, self.num_timesteps)
        composed = (not (isinstance(base, str) and base == "null")) or bool(also) or self._per_sample(guidance_scale)
        interval, phi = self._guidance_args(None if composed else guidance_scale,
                                            None if composed else guidance_interval,
                                            0.0 if composed else guidance_rescale, self.num_timesteps)
        device = self.device
        items = self._norm_counts(class_counts)
        y_list: List[int] = []
        for cls, num in items:
            y_list += [cls] * num
        B = len(y_list)
        geom = self._geom_args(geom_scale, B, model, guidance_scale, guidance_interval, guidance_rescale, base, also,
                               cond)
        y = torch.tensor(y_list, device=device, dtype=torch.long)
        vals, msk = self._build_cond(y_list, cond, cond_mask, key_order, class_keys, device)
        compose = self._compose_args(y_list, vals, msk, guidance_scale, base, also, guidance_interval,
                                     guidance_rescale, null_label, key_order, class_keys, device)
        pag = self._pag_args(pag_scale, pag_blocks, y_list, vals, msk, guidance_scale, compose, model,
                             guidance_interval, guidance_rescale, geom_scale, null_label, device)
        if pag is not None:
            compose = pag[0]
        cache = self._cache_args(cache_interval, model, composed, pag is not None, geom is not None, guidance_interval,
                                 mode is None and not composed and not float(guidance_scale or 0) > 0)

        known, entry = None, {}
        if start_latent is not None:
            if init_latent is not None or mask is not None:
                raise ValueError("`start_latent` excludes `init_latent` and `mask`")
            if mode is None:
                raise ValueError('`start_latent` needs sampler="ddim" or "dpmpp_2m"')
            x, _, _, (C, Hlat, Wlat) = self._known_inputs(start_latent, None, strength, B, z_shape)
            x = x.to(device)  # (the latent as it is: nothing is drawn for x_T)
            entry = dict(start=self._known_start(strength, mode[1]))
        else:
            known = self._known_inputs(init_latent, mask, strength, B, z_shape)
            if known is not None:
                C, Hlat, Wlat = known[3]
            elif z_shape is None:
                if vae is None:
                    raise ValueError("z_shape 省略時は vae が必要です。")
                C, Hlat, Wlat = self._latent_shape(vae, dummy_input_hw, device)
            else:
                C, Hlat, Wlat = z_shape
            x = self._randn((B, C, Hlat, Wlat), device)
        x = self._run_cond_loop(model, x, y, vals, msk, guidance_scale, null_label, progress, mode,
                                known=known[:3] if known is not None else None, interval=interval, rescale=phi,
                                compose=compose, **({} if geom is None else dict(geom=geom)),
                                **({} if pag is None else dict(perturb=pag[1])), **entry,
                                **({} if cache == 1 else dict(cache=cache)))
        if vae is None:
            return x
        if torch.cuda.is_available():
            torch.cuda.empty_cache()
        return self._decode(vae, x, to_pil)

    def invert_latent_cond(self, model, init_latent, class_counts, steps, strength=None, refine=0,
                           guidance_scale: float = 3.0, null_label: int = 0, cond=None, cond_mask=None,
                           key_order: Optional[List[str]] = None, class_keys: Optional[Dict[int, List[str]]] = None,
                           progress: bool = False):
        """DDIM inversion: the probability-flow ODE walked upwards from the latent z0 = init_latent
        ((B,C,h,w), (1,C,h,w) or (C,h,w), broadcast to the batch of class_counts) under the condition that
        sample_latent_cond's class_counts / cond / cond_mask / key_order / class_keys describe.  Returns
        the latent at position p0 = min(S, max(1, floor(strength S + 0.5))) (S for strength None) of
        ddim_timesteps(steps) — fp32, z0's shape — which sample_latent_cond(..., start_latent=it,
        strength=strength, sampler="ddim", steps=steps) walks back down, under the same condition to
        reconstruct z0 or under another one to edit it.  refine = R >= 0: R fixed-point refinements per
        position (invert_tables), R + 1 network evaluations each; R = 0 is the plain inversion, which
        reconstructs poorly under CFG, and every refinement closes the gap by a roughly constant factor.
        A dmx network on the GPU with guidance_scale > 0 runs whole chunks on the device; guidance 0 and
        foreign models step on the host.  Nothing is drawn: the global RNG state is untouched.  Every
        argument violation raises ValueError."""
        T = int(self.num_timesteps)
        if isinstance(steps, bool) or not isinstance(steps, int) or not 1 <= steps <= T:
            raise ValueError(f"steps must be an int in [1, {T}] (got {steps!r})")
        if isinstance(refine, bool) or not isinstance(refine, int) or refine < 0:
            raise ValueError(f"refine must be an int >= 0 (got {refine!r})")
        self._known_start(strength, steps)
        try:
            g = float(guidance_scale)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_scale must be one finite float >= 0 (got {guidance_scale!r})") from None
        if not (math.isfinite(g) and g >= 0):
            raise ValueError(f"guidance_scale must be one finite float >= 0 (got {guidance_scale!r})")
        if init_latent is None:
            raise ValueError("init_latent (the latent to invert) is required")
        device = self.device
        y_list: List[int] = []
        for cls, num in self._norm_counts(class_counts):
            y_list += [cls] * num
        z0 = self._known_inputs(init_latent, None, None, len(y_list), None)[0]
        y = torch.tensor(y_list, device=device, dtype=torch.long)
        vals, msk = self._build_cond(y_list, cond, cond_mask, key_order, class_keys, device)
        x = self._run_cond_loop(model, z0.to(device), y, vals, msk, g, null_label, progress,
                                ("invert", steps, strength, refine))
        return x.to(torch.float32)

    def _plan(self, x, mode, guidance_scale, known=None, interval=None, rescale=0.0, compose=None,
              rows=None, geom=None, perturb=None, start=None, cache=1) -> _SamplerPlan:
        """The plan of a sampling call whose x_T draw is x, on x's device.
        mode: _sampler_mode's result.  interval, rescale: _guidance_args' (t_lo, t_hi) or None and phi.
        compose: _compose_args' tables or None; a composed plan has no scale, interval or rescale.
        known = (z0, mask or None, strength) (_known_inputs) or None: x is the call's fixed draw e0 and
        the loop enters at p0 = _known_start.  plan.x_start then holds x's values for p0 = total, else
        the blend's kn one table row up (position p0 + 1 arrives at tau_p0), written to a new tensor;
        without a mask no step is blended.
        rows = (s, e): a shard — x holds the rows [s, e) of the global draw, and the plan takes those
        rows of z0 and the mask and the columns [:, s:e] of the compose tables.
        geom: _geom_args' scale row or None; the plan carries its rows and the sig table of the rule
        (geom_sig for ddpm, the schedule's k_e otherwise), converted once: a loop's graphs hold their pointers.
        perturb: _pag_args' (blocks, branches) or None, for the compose tables that came with it; the
        pair does not depend on the shard.
        start = p0 (a strided rule, no `known`): x is no draw but the latent the loop starts from, as it
        is, at position p0 (sample_latent_cond's start_latent).
        mode ("invert", S, strength, R): the plan of invert_latent_cond — x is z0, the schedule is
        invert_tables' and the counter walks its N rows down; it takes none of the other parts.
        cache = N (_cache_args): feature caching with a refresh every N-th position of a guard chunk; it
        takes no composition, geometry or perturbed-attention guidance, guidance interval or inversion."""
        dev = x.device
        rule = "ddpm" if mode is None else mode[0]
        tau = self._mode_timesteps(mode)
        cut = slice(None) if rows is None else slice(*rows)
        plan = _SamplerPlan(rule, start=len(tau), draws=rule == "ddpm" or (rule == "ddim" and mode[2] > 0),
                            rows=rows, x_start=x)
        if isinstance(cache, bool) or cache != 1:
            if isinstance(cache, bool) or not isinstance(cache, int) or cache < 1:
                raise ValueError(f"cache must be an int >= 1 (got {cache!r})")
            for nm, v in (("composition", compose), ("geometry guidance", geom),
                          ("perturbed-attention guidance", perturb), ("guidance interval", interval),
                          ("inversion", True if rule == "invert" else None)):
                if v is not None:
                    raise ValueError(f"a cached plan (cache_interval > 1) takes no {nm}")
            plan.cache = cache
        if perturb is not None:
            if compose is None:
                raise ValueError("perturb belongs to the compose tables of _pag_args")
            plan.perturb = (int(perturb[0]), int(perturb[1]))
        if compose is not None:  # converted once: a loop's graphs hold their pointers
            plan.compose = tuple(c[:, cut].to(dev).contiguous() for c in compose)
        else:
            plan.scale = float(guidance_scale) if guidance_scale else 0.0
            plan.rescale = float(rescale)
            plan.run_g = True if interval is None else self._guided_run(tau, interval)
        if known is not None:
            z0, kmask, strength = known
            total, plan.start = len(tau), self._known_start(strength, len(tau))
            if x.shape[0] > 0 and (plan.start < total or kmask is not None):
                e0 = x.to(torch.float32).contiguous()
                z0 = z0[cut].to(dev)
                q_a, q_e = self.known_tables(tau, dev)
                if plan.start < total:
                    pos = torch.full((1,), plan.start + 1, dtype=torch.long, device=dev)
                    plan.x_start = _engine.known_blend(z0, pos, (z0, e0, None, q_a, q_e))
                else:  # (e0 stays a constant of the loop: in-place steps must not write it)
                    plan.x_start = e0.clone()
                if kmask is not None:
                    plan.known = (z0, e0, kmask[cut].to(dev), q_a, q_e)
        if start is not None:
            if known is not None or rule not in ("ddim", "dpm"):
                raise ValueError("a start position belongs to a strided loop without a known region")
            plan.start = int(start)
        if rule == "ddpm":
            plan.tables = self.coef_tables(dev, clamp_prev=True)
        elif rule == "ddim":
            plan.sched = self.ddim_tables(mode[1], mode[2], dev)
        elif rule == "invert":
            if not (known is None and interval is None and compose is None and geom is None and not rescale > 0):
                raise ValueError("inversion takes no known region, interval, rescale, composition or geometry guidance")
            plan.sched = self.invert_tables(mode[1], mode[2], mode[3], dev)
            plan.start = int(plan.sched[0].numel())
        else:  # (a loop entering at p0 < S: that row is first-order)
            entered = known is not None or start is not None
            plan.sched = self.dpm_tables(mode[1], mode[2], dev, plan.start if entered else None)
        if geom is not None:
            sig = self.geom_sig(dev) if rule == "ddpm" else self._sched_sig(plan.sched)
            plan.geom = (geom[cut].to(device=dev, dtype=torch.float32).contiguous(), sig)
        return plan

    def _device_chunks(self, nm, plan, x, y, null_label, vals, msk, hist, seed, bar=None):
        """The chunk runner of the device loop on x: Philox noise, hipGraph replay, the position scalar
        decremented in-graph — it runs on across a chunk's segments (plan.segments).  An empty shard
        launches nothing.  nm: the native model, told this Diffuser's prediction by the caller (_native)."""
        t_dev = torch.full((1,), plan.start, device=x.device, dtype=torch.long)

        def run(i_from, i_to, x):
            if x.shape[0] > 0:
                t_dev.fill_(i_from)
                for a, b, guided in plan.segments(i_from, i_to):
                    nm.sample_loop(x, t_dev, y, null_label, vals, msk, plan.guidance(guided), plan.tables, a - b,
                                   **plan.kwargs(guided, hist, seed=seed, use_graph=self.use_graph))
            if bar is not None:
                bar.update(i_from - i_to)
            return x
        return run

    def _run_cond_loop(self, model, x, y, vals, msk, guidance_scale, null_label, progress, mode=None, known=None,
                       interval=None, rescale=0.0, compose=None, geom=None, perturb=None, start=None, cache=1):
        """The T loop (diff.py:328-344) over the call's plan (_plan), range-guarded in chunks
        (_guarded_loop): the counter walks timesteps, or the positions of a strided schedule, down
        from plan.start, and a replayed chunk restarts from the x and the solver history it started
        with.  A dmx network with guidance (or a composed call) in device-noise mode runs whole chunks
        on the device (_device_chunks); every other case steps on the host (_step).  An inversion
        (mode "invert") draws nothing and takes the device loop in either noise mode; its source latent
        travels in the history slot, so a replayed chunk restarts from its x and its src.
        cache = N > 1 (_cache_args): every guard chunk starts with a refresh step and refreshes every N-th
        step after it — the device loop passes phase 0 per chunk call, the host loop the step's offset."""
        plan = self._plan(x, mode, guidance_scale, known, interval, rescale, compose, geom=geom, perturb=perturb,
                          **({} if start is None else dict(start=start)), **({} if cache == 1 else dict(cache=cache)))
        x = plan.x_start
        hist = plan.new_hist(x)
        guard = self._guard_target(model, x)
        native = _native_kind(model) in (1, 2) and x.is_cuda and (plan.compose is not None or plan.scale > 0)
        device_loop = native and (self.noise_source == "device" or plan.rule == "invert")
        bar = tqdm(total=plan.start, desc="Sampling (cond+numeric)") if progress else None
        if device_loop:
            x = x.contiguous().clone()
            seed = 0 if plan.rule in ("dpm", "invert") else self._seed()  # (these draw nothing)
            run = self._device_chunks(self._native(model), plan, x, y, null_label, vals.float().contiguous(),
                                      msk.float().contiguous(), hist, seed, bar)
        else:
            def step_chunk(i_from, i_to, x):
                for i in range(i_from, i_to, -1):  # i in [1, T]: the public steps' asserts hold by construction
                    t = torch.full((x.shape[0],), i, device=x.device, dtype=torch.long)
                    x = self._step(model, x, t, plan, plan.guided(i), y, null_label, vals, msk, hist,
                                   **({} if plan.cache == 1 else dict(phase=i_from - i)))
                    if bar is not None:
                        bar.update(1)
                return x
            run = self._prefetching(step_chunk, model, x, plan.draws)
        with torch.no_grad():
            x = self._guarded_loop(run, x, plan.start, guard, hist, inplace=device_loop)
        if bar is not None:
            bar.close()
        return x
