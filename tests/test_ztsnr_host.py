"""CPU: the zero-terminal-SNR schedule and the x0-form — the rescaled tables, the decisions at
ab_T = 0, the constructor's rules, and the torch restatements of tests/rules_x0.py against the eps-form rules
of oracle/rules.py (float64, an ordinary schedule) and against the float64 direct form (fp32, the rescaled
schedule)."""
import os

import pytest
import torch

import diff
import rules_x0
from conftest import REPO
from oracle import ref, rules
from rules_x0 import rel

T = 1000


def dz(n=T, **kw):
    return diff.Diffuser(n, prediction="v", zero_terminal_snr=True, **kw)


def dv(n=T, **kw):
    return diff.Diffuser(n, prediction="v", **kw)


# ---- the schedule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 50, 20, 2])
def test_rescaled_schedule(n):
    d, plain = dz(n), dv(n)
    a, ab = d._host
    _, a0, ab0 = ref.schedule(n)
    assert torch.equal(plain._host[0], a0) and torch.equal(plain._host[1], ab0)  # the unrescaled one is the reference's
    assert ab.dtype == torch.float32 and a.dtype == torch.float32
    assert float(ab[-1]) == 0.0 and float(a[-1]) == 0.0
    assert torch.equal(ab[0], ab0[0]) and torch.equal(a[0], ab0[0])
    assert bool((ab[1:] < ab[:-1]).all())
    # Algorithm 1 of Lin et al. 2023 in fp32, and the alphas of the rescaled ab (no second cumprod)
    s = torch.sqrt(ab0)
    s = (s - s[-1]) * s[0] / (s[0] - s[-1])
    assert torch.equal(ab[1:], (s * s)[1:])
    assert torch.equal(a[1:], ab[1:] / ab[:-1])
    assert torch.equal(d.alpha_bars.cpu(), ab) and torch.equal(d.alphas.cpu(), a) and torch.equal(d.betas.cpu(), 1 - a)
    assert d._host[1] is ab and d.zero_terminal_snr and d.x0_form
    # every table reads it: the noising tables are its roots
    sa, s1 = d.noise_tables("cpu")
    assert torch.equal(sa, torch.sqrt(ab)) and torch.equal(s1, torch.sqrt(1 - ab))
    assert float(sa[-1]) == 0.0 and float(s1[-1]) == 1.0


def test_defaults_change_no_table():
    a, b, c = dv(), dv(zero_terminal_snr=False, x0_form=False), dv(x0_form=True)
    e = diff.Diffuser(T)
    assert not a.zero_terminal_snr and not a.x0_form and not e.x0_form and c.x0_form and not c.zero_terminal_snr
    _, a0, ab0 = ref.schedule(T)

    def tables(d):
        out = list(d._host) + list(d.coef_tables("cpu")) + list(d.coef_tables("cpu", False))
        out += list(d.ddim_tables(50, 0.5)) + list(d.dpm_tables(20, "logsnr")) + list(d.dpm_tables(20, "uniform", start=7))
        out += list(d.invert_tables(10, None, 1)) + list(d.known_tables((1, 5, 900, 1000))) + list(d.noise_tables("cpu"))
        out += list(d.pred_tables("cpu")) + [d.geom_sig("cpu"), d.loss_weights("min_snr"), d._sched_sig(d.ddim_tables(50, 0.5))]
        return out + [torch.tensor(d.dpm_timesteps(20)), torch.tensor(d.dpm_timesteps(1000))]
    for other in (b, c):
        for u, v in zip(tables(a), tables(other)):
            assert u.dtype == v.dtype and torch.equal(u, v)
    assert torch.equal(e._host[0], a0) and torch.equal(e._host[1], ab0) and torch.equal(a._host[1], ab0)
    # today's expressions, written out: the v-mode sig and the logsnr grid
    assert torch.equal(a.geom_sig("cpu"), torch.sqrt(1 - ab0) / torch.sqrt(ab0))
    lam = 0.5 * torch.log(ab0.double() / (1 - ab0.double()))
    grid = lam[0] + torch.arange(20, dtype=torch.float64) / 19 * (lam[-1] - lam[0])
    tau = [int(torch.argmin(torch.abs(lam - g))) + 1 for g in grid]
    assert a.dpm_timesteps(20)[1:-1] == tau[1:-1]


def test_constructor_rules():
    for kw in (dict(prediction="eps", zero_terminal_snr=True), dict(zero_terminal_snr=True),
               dict(prediction="eps", x0_form=True), dict(x0_form=True),
               dict(prediction="v", zero_terminal_snr=True, x0_form=False)):
        with pytest.raises(ValueError):
            diff.Diffuser(T, **kw)
    with pytest.raises(ValueError):
        diff.Diffuser(1, prediction="v", zero_terminal_snr=True)
    with pytest.raises(TypeError):
        diff.Diffuser(1000, 1e-4, 0.02, "cpu", "v")  # keyword-only
    assert dz(2).x0_form and dz(x0_form=True).x0_form and dz(x0_form=None).x0_form
    assert not diff.Diffuser(T, prediction="eps", x0_form=False).x0_form


# ---- x0_tables --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [dz, dv])
def test_x0_tables(make):
    d = make(x0_form=True)
    d_s, d_d = d.x0_tables("cpu")
    a, ab = (v.double() for v in d._host)
    abp = torch.cat([torch.ones(1, dtype=torch.float64), ab[:-1]])
    assert d_s.dtype == torch.float32 and torch.equal(d_s, torch.sqrt(abp).float())
    assert torch.equal(d_d, ((1 - abp) * torch.sqrt(a) / torch.sqrt(1 - ab)).float())
    assert float(d_s[0]) == 1.0 and float(d_d[0]) == 0.0
    assert torch.isfinite(d_s).all() and torch.isfinite(d_d).all()
    if d.zero_terminal_snr:
        assert float(d_d[-1]) == 0.0 and float(d_s[-1]) > 0.0
    else:  # the posterior mean of the eps-form, in float64: mu = (x - c1 eps) / c2 with x = sqrt(ab) x0 + sqrt(1-ab) eps
        g = torch.Generator().manual_seed(0)
        x0, eps = torch.randn((T, 64), generator=g, dtype=torch.float64), torch.randn((T, 64), generator=g, dtype=torch.float64)
        col = lambda v: v.view(-1, 1)  # noqa: E731
        x = col(torch.sqrt(ab)) * x0 + col(torch.sqrt(1 - ab)) * eps
        # the identity needs ab_t = a_t ab_prev: exact with the alphas the alpha_bars imply ...
        ac = ab / abp
        mu = (x - col((1 - ac) / torch.sqrt(1 - ab)) * eps) / col(torch.sqrt(ac))
        mine = col(torch.sqrt(abp)) * x0 + col((1 - abp) * torch.sqrt(ac) / torch.sqrt(1 - ab)) * eps
        assert rel(mine, mu) < 1e-13
        # ... and as close as the fp32 schedule is to itself with the tabulated ones (the cumprod and the alphas
        # are each rounded to fp32 once: a_t ab_prev / ab_t - 1 is a few 2^-24, and so is the distance)
        assert float((a * abp / ab - 1).abs().max()) < 3 * 2.0 ** -24
        mu = (x - col((1 - a) / torch.sqrt(1 - ab)) * eps) / col(torch.sqrt(a))
        mine = col(d_s.double()) * x0 + col(d_d.double()) * eps
        assert rel(mine, mu) < 3 * 2.0 ** -24
    assert d.x0_tables("cpu")[0] is d_s  # cached


# ---- the decisions at ab_T = 0 ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 50])
def test_dpm_timesteps_and_tables(n):
    d = dz(n)
    assert d.dpm_timesteps(1) == [n]
    assert d.dpm_timesteps(n) == list(range(1, n + 1))
    for S in (2, 3, 5, 17, n - 1):
        tau = d.dpm_timesteps(S)
        assert len(tau) == S and tau[-1] == n and tau[0] >= 1
        assert all(v > u for u, v in zip(tau, tau[1:]))
        assert d.dpm_timesteps(S, "uniform") == d.ddim_timesteps(S)
    # the interior points: uniform in lam between lam[1] and lam[T-1]
    ab = d._host[1].double()
    lam = (0.5 * torch.log(ab / (1 - ab)))[:n - 1]
    tau = d.dpm_timesteps(5)
    grid = lam[0] + torch.arange(4, dtype=torch.float64) / 3 * (lam[-1] - lam[0])
    assert tau[:4] == [int(torch.argmin(torch.abs(lam - g))) + 1 for g in grid] and tau[3] == n - 1
    for S, spacing, start in ((1, "logsnr", None), (2, "logsnr", None), (5, "logsnr", None), (5, "uniform", None),
                              (n, "logsnr", None), (5, "logsnr", 3), (5, "uniform", 4)):
        tabs = d.dpm_tables(S, spacing, "cpu", start)
        for v in tabs[1:]:
            assert v.dtype == torch.float32 and torch.isfinite(v).all()
        k_a, k_c, k_p = tabs[2], tabs[4], tabs[5]
        assert float(k_a[-1]) == 0.0
        for r in range(max(S - 2, 0), S):  # the terminal row and the row after it: first-order, +0.0
            assert float(k_p[r]) == 0.0 and not bool(torch.signbit(k_p[r]))
        if S >= 3 and start is None:
            m = torch.sqrt(ab[tabs[0][S - 3] - 1]) - torch.sqrt(1 - ab[tabs[0][S - 3] - 1]) / torch.sqrt(1 - ab[tabs[0][S - 2] - 1]) \
                * torch.sqrt(ab[tabs[0][S - 2] - 1])
            assert float(k_c[S - 2]) == float(m.float())
        if S >= 4 and start is None:
            assert float(k_p[1]) != 0.0  # the rows below stay second-order


def test_ddim_and_invert_tables_finite():
    d = dz()
    for S, eta in ((1, 0.0), (5, 0.0), (5, 1.0), (50, 0.5), (T, 1.0)):
        tabs = d.ddim_tables(S, eta)
        assert int(tabs[0][-1]) == T and float(tabs[2][-1]) == 0.0 and float(tabs[1][-1]) == 1.0
        for v in tabs[1:]:
            assert torch.isfinite(v).all()
    for v in d.invert_tables(5, None, 1)[1:3]:
        assert torch.isfinite(v).all()
    for v in d.known_tables(d.ddim_timesteps(5)) + d.coef_tables("cpu")[::2]:
        assert torch.isfinite(v).all()


def test_geom_sig_is_zero_at_the_terminal_row():
    d = dz()
    sig = d.geom_sig("cpu")
    ab = d._host[1]
    assert torch.isfinite(sig).all() and float(sig[-1]) == 0.0
    assert torch.equal(sig[:-1], (torch.sqrt(1 - ab) / torch.sqrt(ab))[:-1])
    sched = d.ddim_tables(5, 0.0)
    ss = d._sched_sig(sched)
    assert torch.isfinite(ss).all() and float(ss[-1]) == 0.0 and torch.equal(ss[:-1], (sched[1] / sched[2])[:-1])
    assert float(ss[-2]) > 1.0  # the second position shows the divided sig


def test_min_snr_weight_is_zero_at_T():
    d = dz()
    w = d.loss_weights("min_snr", 5.0)
    assert torch.isfinite(w).all() and float(w[-1]) == 0.0 and bool((w[:-1] > 0).all())
    snr = d._host[1].double() / (1 - d._host[1].double())
    assert torch.equal(w, (torch.clamp(snr, max=5.0) / (snr + 1)).float())
    assert torch.equal(d.loss_weights("uniform"), torch.ones(T))


# ---- the restatements ---------------------------------------------------------------------------------------
def tables64(d, t, s, u=None, eta=0.0, implied=True):
    """Float64 rows of the three rules for steps t -> s ((N,) long; s = 0: alpha_bar 1), u the step before (DPM),
    from the Diffuser's fp32 alpha_bars: ((p_o, p_x) per timestep, ddim sched, dpm sched, (a, ab, d_s, d_d, sd)).
    The alphas are those the alpha_bars imply, a_t = ab_t / ab_prev in float64: the posterior mean's two forms are
    the same map only on a schedule that is consistent with itself (the fp32 tables are, to a few 2^-24:
    test_x0_tables)."""
    ab1 = torch.cat([torch.ones(1, dtype=torch.float64), d._host[1].double()])
    a = ab1[1:] / ab1[:-1] if implied else d._host[0].double()  # (else: the Diffuser's own fp32 alphas)
    ab, ab_t, ab_s = ab1[1:], ab1[t], ab1[s]
    k_e, k_a = torch.sqrt(1 - ab_t), torch.sqrt(ab_t)
    sigma = eta * torch.sqrt((1 - ab_s) / (1 - ab_t)) * torch.sqrt(1 - ab_t / ab_s)
    ddim = (t, k_e, k_a, torch.sqrt(ab_s), torch.sqrt(torch.clamp(1 - ab_s - sigma * sigma, min=0.0)), sigma)
    k_x = torch.sqrt(1 - ab_s) / k_e
    m = torch.sqrt(ab_s) - k_x * k_a
    k_c, k_p = m.clone(), torch.zeros_like(m)
    if u is not None:
        lam = lambda v: 0.5 * torch.log(v / (1 - v))  # noqa: E731
        r = (lam(ab_t) - lam(ab1[u])) / (lam(ab_s) - lam(ab_t))
        first = (s == 0) | (u <= t)  # (first-order rows, as in dpm_tables: the last step, lam[0] = inf, and a first one)
        k_c, k_p = torch.where(first, m, m * (1 + 1 / (2 * r))), torch.where(first, torch.zeros_like(m), -m / (2 * r))
    dpm = (t, k_e, k_a, k_x, k_c, k_p)
    abp = ab1[:-1]
    post = (a, ab, torch.sqrt(abp), (1 - abp) * torch.sqrt(a) / torch.sqrt(1 - ab), rules_x0.posterior_sd(a, ab))
    return (torch.sqrt(ab), torch.sqrt(1 - ab)), ddim, dpm, post


def test_float64_x0_form_equals_the_eps_form():
    """On an ordinary schedule the two forms are the same map of (x, v): float64, 1e-12."""
    d = dv(x0_form=True)
    t = torch.tensor([1, 2, 20, 500, 900, 980, 999, 1000, 1000, 600])
    s = torch.tensor([0, 1, 0, 480, 899, 960, 998, 999, 980, 300])
    u = torch.tensor([5, 9, 40, 520, 901, 1000, 1000, 1000, 1000, 900])
    g = torch.Generator().manual_seed(1)
    shape = (t.numel(), 4, 8, 8)
    x, out, nz, hist = (torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(4))
    pos = torch.arange(1, t.numel() + 1)
    for eta in (0.0, 1.0):
        (p_o, p_x), ddim, dpm, (a, ab, d_s, d_d, sd) = tables64(d, t, s, u, eta)
        eps_e = rules.to_eps(out, x, t, p_o, p_x)
        x0, eps = rules_x0.x0_split(out, x, t, p_o, p_x)
        assert torch.equal(eps, eps_e)
        pairs = [("ddim", rules_x0.ddim_x0_update(x0, eps, pos, ddim, nz), rules.ddim_update(x, eps_e, pos, ddim, nz)),
                 ("ddpm", rules_x0.ddpm_x0_update(x0, eps, t, d_s, d_d, sd, nz), ref.ddpm_update(x, eps_e, t, a, ab, nz))]
        y1, h1 = rules_x0.dpm_x0_update(x, x0, pos, dpm, hist)
        y0, h0 = rules.dpm_update(x, eps_e, pos, dpm, hist)
        pairs += [("dpm", y1, y0), ("dpm hist", h1, h0)]
        for name, mine, theirs in pairs:
            err = rel(mine, theirs)
            print(f"[x0-form == eps-form, float64, eta={eta}] {name}: {err:.3e}")
            assert err < 1e-12, (name, err)
    with rules_x0.x0_rules(p_o, p_x, d_s, d_d):  # the swapped rules are restored
        assert rules.ddim_update is not ddim_saved and ref.ddpm_update is not ddpm_saved
    assert rules.ddim_update is ddim_saved and ref.ddpm_update is ddpm_saved and rules.dpm_update is dpm_saved


ddim_saved, dpm_saved, ddpm_saved = rules.ddim_update, rules.dpm_update, ref.ddpm_update


def test_fp32_x0_form_on_the_rescaled_schedule():
    """fp32 tables and fp32 arithmetic, one rounding per op, against the float64 direct form on the same fp32
    schedule: 2e-7, three times the worst figure measured (7.2e-8).  A contracted or re-ordered restatement,
    or one that went through eps / k_a, does not stay there (the eps-form is non-finite at t = T)."""
    d = dz()
    g = torch.Generator().manual_seed(2)
    x, out, nz = (torch.randn((1, 4, 64, 64), generator=g) for _ in range(3))
    p_o, p_x = d.pred_tables("cpu")
    d_s, d_d = d.x0_tables("cpu")
    sd = d.coef_tables("cpu")[2]
    worst = 0.0
    for tt in (1, T // 2, T - 1, T):
        t = torch.tensor([tt])
        x0, eps = rules_x0.x0_split(out, x, t, p_o, p_x)
        assert x0.dtype == torch.float32 and torch.isfinite(x0).all() and torch.isfinite(eps).all()
        for stride in (1, 20, tt):
            s = torch.tensor([max(tt - stride, 0)])
            (q_o, q_x), ddim64, _, (a, ab, e_s, e_d, sd64) = tables64(d, t, s, implied=False)
            x064, eps64 = rules_x0.x0_split(out.double(), x.double(), t, q_o, q_x)
            one = torch.tensor([1])
            ddim32 = tuple(v if v.dtype == torch.long else v.float() for v in ddim64)
            got = rules_x0.ddim_x0_update(x0, eps, one, ddim32, None)
            err = rel(got, rules_x0.ddim_x0_update(x064, eps64, one, ddim64, None))
            worst = max(worst, err)
            assert got.dtype == torch.float32 and err < 2e-7, ("ddim", tt, stride, err)
        got = rules_x0.ddpm_x0_update(x0, eps, t, d_s, d_d, sd, nz)
        err = rel(got, rules_x0.ddpm_x0_update(x064, eps64, t, e_s, e_d, sd64, nz.double()))
        worst = max(worst, err)
        assert got.dtype == torch.float32 and err < 2e-7, ("ddpm", tt, err)
    print(f"[fp32 x0-form vs float64, rescaled schedule] worst rel-L2 = {worst:.3e}")
    # the eps-form at the terminal step: not finite
    sched = d.ddim_tables(50, 0.0)
    t = torch.tensor([T])
    bad = rules.ddim_update(x, rules.to_eps(out, x, t, p_o, p_x), torch.tensor([50]), sched, None)
    assert not torch.isfinite(bad).all()
    # and the rules' own tables at the terminal row: x0 = -out, eps = x exactly
    x0, eps = rules_x0.x0_split(out, x, t, p_o, p_x)
    assert torch.equal(x0, -out) and torch.equal(eps, x)


# ---- the ABI ------------------------------------------------------------------------------------------------
NEW = {"dmx_model_set_prediction_x0": 7, "dmx_pred_split": 14}


def test_header_and_bindings_name_the_new_symbols():
    import ctypes
    from dmx import _lib
    hdr = open(os.path.join(REPO, "include", "dmx.h")).read()
    bound = {n: (r, a) for n, r, a in _lib.SIGNATURES}
    for sym, nargs in NEW.items():
        assert f"int {sym}(" in hdr, sym
        assert sym in bound and len(bound[sym][1]) == nargs, sym
    assert "#define DMX_PRED_V_X0 2" in hdr
    lib = _lib.load()
    for sym in NEW:
        assert hasattr(lib, sym), sym
    assert lib.dmx_abi_version() == 1
    assert ctypes.sizeof(_lib.StepArgs) == 144 and ctypes.sizeof(_lib.NoiseArgs) == 160
    assert lib.dmx_model_set_prediction_x0(None, None, None, None, None, 1000, None) == _lib.DMX_E_ARG
    assert lib.dmx_pred_split(None, None, None, 1, None, None, 1000, 1, 4, 8, 8, None, None, None) == _lib.DMX_E_ARG
    assert lib.dmx_model_set_prediction(None, 2, None, None, 1000, None) == _lib.DMX_E_ARG  # not a kind of that entry
    assert lib.dmx_last_error()


def test_python_entries():
    import inspect
    from dmx import engine
    from dmx._lib import DmxUnavailable
    d = dz()
    x = torch.zeros((2, 4, 8, 8))
    with pytest.raises(DmxUnavailable):
        engine.pred_split(x, x, torch.ones(2, dtype=torch.long), *d.pred_tables("cpu"))
    sig = inspect.signature(engine.NativeModel.set_prediction).parameters
    assert sig["d_s"].kind is inspect.Parameter.KEYWORD_ONLY and sig["d_d"].default is None
    assert engine.NativeModel.PREDICTIONS == {"eps": 0, "v": 1} and engine.NativeModel.PRED_V_X0 == 2

    class Stub:  # a stand-in without set_prediction reads eps
        device = "cpu"
    with pytest.raises(TypeError):
        d._set_prediction(Stub())
    seen = []

    class Takes:
        device = "cpu"

        def set_prediction(self, kind, p_o=None, p_x=None, *, d_s=None, d_d=None):
            seen.append((kind, p_o, p_x, d_s, d_d))
    d._set_prediction(Takes())
    dv()._set_prediction(Takes())
    assert seen[0][0] == "v" and seen[0][3] is d.x0_tables("cpu")[0] and seen[0][4] is d.x0_tables("cpu")[1]
    assert seen[1][0] == "v" and seen[1][3] is None and seen[1][4] is None
    # a foreign model's operands cannot be converted for the x0-form
    with pytest.raises(TypeError):
        d._to_eps(x, None, 0.0, x, torch.ones(2, dtype=torch.long))


def test_the_standalone_argument_check_calls_the_new_rules():
    """tools/prediction_args_check.cpp is built and run under the host sanitizers by tests/test_vpred_host.py;
    here: it calls the rules of the two new entries."""
    text = open(os.path.join(REPO, "tools", "prediction_args_check.cpp")).read()
    for rule in ("set_prediction_x0_error(", "pred_split_error("):
        assert rule in text, rule
