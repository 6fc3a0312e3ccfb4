"""kernel_plan.json — the ordered (kernel, layer) launch labels of one eager CFG step, for
tests/test_gpu_kernel_plan.py.

The fixture pins launch DECISIONS across a refactor of the code that takes them, so it must come
from the library of the commit before that refactor (the parent build), never from the code under
test: build the parent's sources next to libdmx.so and select them with DMX_LIB, on an MI355X,

    python diffusion-model_amd/dmx/build.py --out libparent.so     (in a checkout of the parent)
    DMX_LIB=libparent.so python tests/golden/make_kernel_plan.py

Regenerate only when a change is MEANT to move a launch (a new kernel, a new threshold), again from
the last commit whose decisions were reviewed, and say so in that commit."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(REPO, "diffusion-model_amd"), REPO, os.path.join(REPO, "tests")]

import torch  # noqa: E402

import test_gpu_kernel_plan as T  # noqa: E402
from dmx import synth  # noqa: E402


def main() -> None:
    dev = torch.device("cuda:0")
    model, diffuser = T.model_and_diffuser(dev, synth.unet_cond_geom_weights(0))
    plans = {}
    for prec in T.PRECISIONS:
        for B, hw in T.SHAPES:
            plans[T.case_id(prec, B, hw)] = T.record_plan(model, diffuser, prec, B, hw, dev)
            print(T.case_id(prec, B, hw), len(plans[T.case_id(prec, B, hw)]), "launches", flush=True)
    note = ("Recorded by tests/golden/make_kernel_plan.py, never from the code under test (DMX_LIB=%s): the B1, B5 "
            "and B32 32x32, B32 28x28 and B3 16x16 plans with the library built from the parent of the conv-plan "
            "refactor; the B17 32x32 and B21 40x40 plans, added with tests/test_gpu_forward_classes.py, with the "
            "library built from the parent of that change, which reproduced the earlier plans exactly."
            % os.environ.get("DMX_LIB", "libdmx.so"))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "kernel_plan.json")
    with open(out, "w") as f:
        json.dump({"note": note, "plans": plans}, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
