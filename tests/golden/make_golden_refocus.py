#!/usr/bin/env python3
"""Generate tests/golden/g20_refocus_stack.npz by running the REAL reference on PyTorch-CPU.

Runs only where the reference tree is present (REF below, read-only); same import recipe as make_golden.py.  The reference's own
eval-time PostProcess (blurry_edges_test.py:12-100) in float64 - helper tensors cast to double as make_golden.py's G16 does
(`_as_double_global`) - on G6's inputs (synth.synthetic_image_pair(147, 147), synth.plausible_params12(4096, name="g6_est")),
densify = None, with args.rho_prime set in turn to the three optical powers below: focus at 2.30, 0.95 and 0.65 m, i.e. beyond,
inside and in front of the 0.75 .. 1.18 m the models are trained on.  Stored as float32 (6e-8 relative, far below the 1e-4 the
planes are compared at): the powers, the folded refocused image of each and the per-patch refocused render of the 4 x 4 patch
sub-grid [20:24, 30:34] in G16's layout.  Outputs only: inputs are regenerated from be_hip.synth wherever the fixture is used.

usage: python tests/golden/make_golden_refocus.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "g20_refocus_stack.npz")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(ROOT, "blurry-edges_amd"))
from be_hip import synth  # noqa: E402

sys.path.insert(0, REF)
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
for _m in ("models", "utils", "data"):
    assert _m not in sys.modules
import utils as ref_utils                # noqa: E402
assert ref_utils.__file__.startswith(REF)
import blurry_edges_test as ref_test     # noqa: E402

RHO_PRIMES = (9.4928, 10.1106, 10.5964)      # 1 / z + 1 / 0.1104 for z = 2.30, 0.95, 0.65 m


def ref_args():
    argv, sys.argv = sys.argv, ["x"]
    try:
        return ref_utils.get_args("eval")
    finally:
        sys.argv = argv


def as_double_global(helper, dcal):
    """the reference's eval-time helper with every constant tensor cast to float64 (make_golden.py: _as_double_global)"""
    helper.x, helper.y, helper.ridge = helper.x.double(), helper.y.double(), helper.ridge.double()
    helper.sobel_x, helper.sobel_y = helper.sobel_x.double(), helper.sobel_y.double()
    helper.num_patches = helper.num_patches.double()
    dcal.intercept, dcal.theta_mid, dcal.theta_wng = dcal.intercept.double(), dcal.theta_mid.double(), dcal.theta_wng.double()


def main():
    torch.set_num_threads(8)
    a = ref_args()
    a.densify = None
    dev = torch.device("cpu")
    imgs, _ = synth.synthetic_image_pair(147, 147)
    t_img = torch.from_numpy(imgs).double()
    img_patches = torch.nn.Unfold(a.R, stride=a.stride)(t_img).view(2, 3, a.R, a.R, 64, 64)
    p12 = torch.from_numpy(synth.plausible_params12(4096, name="g6_est"))[None].double()
    sub = (slice(20, 24), slice(30, 34))
    f32 = lambda t: (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.float32)
    folds, subs = [], []
    for rho in RHO_PRIMES:
        a.rho_prime = rho
        dcal = ref_utils.DepthEtas(a, dev)
        helper = ref_test.PostProcess(a, dcal, dev)
        as_double_global(helper, dcal)
        helper.img_patches = img_patches.unsqueeze(0)
        est = p12.permute(0, 2, 1).view(1, 12, 64, 64)
        etas = helper.params2etas(est[:, 8:])
        refoc = helper.get_patches(est[:, :8], etas, False)[2]
        folded = helper(p12, img_patches, colors_only=False)
        fold = f32(folded[2])
        folds.append(fold.reshape(3, 147, 147))
        subs.append(f32(refoc[0][..., sub[0], sub[1]]))
    out = dict(rho_primes=np.asarray(RHO_PRIMES, dtype=np.float32), fold_refoc=np.stack(folds), sub_refoc=np.stack(subs))
    assert all(np.isfinite(v).all() for v in out.values())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1024:.1f} KiB): " + ", ".join(f"{k} {v.shape}" for k, v in out.items()))


if __name__ == "__main__":
    main()
