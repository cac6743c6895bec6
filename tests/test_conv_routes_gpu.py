"""Every route and tile the fp32 convolution's planner (be_conv.hip: conv_plan) can choose, at the smallest shapes on both sides of
each threshold: the launches' profile records (kernel id, FLOPs, bytes, executed FLOPs) and the bits of y, against
tests/golden/conv_routes.json.  The golden was recorded on the MI355X with the library of the commit BEFORE the planner existed
(conv_dispatch, 32969ca), from a checkout of that commit:

    python tests/test_conv_routes_gpu.py --record          (this file copied into that checkout; it uses only entry points that
                                                            library has, and writes tests/golden/conv_routes.json there)

Several of these decisions cannot be seen in y: uniform and bordered small tiles, the pixel-major LDS-DMA kernel and the
pixel-major implicit GEMM, the row GEMM and the 128 x 128 tiles give the same bits.  They show in the profile records - a wrong
route is a silent slowdown otherwise.  Inputs and weights are numpy default_rng draws on the CPU.  tests/test_host_cpu.py runs the
planner itself (be_conv_plan_debug, no GPU) over the same cases and holds its kernel ids and executed FLOPs to the same golden."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
DEV = "cuda:0"

# BE_KERNEL_* ids (include/blurry_edges_hip.h)
K128, K96, K64, K32, KROW8, KSMALL, KROWS = 0, 1, 2, 3, 4, 5, 7


def _case(key, shape, kernels, res=False, cin2=0, nbatch=1, scratch=None):
    """shape = (n, h, w, cin, cout, ks); kernels = the kernel ids of its launches; scratch: None | slices of M * cout_pad32 floats"""
    return dict(key=key, shape=shape, kernels=kernels, res=res, cin2=cin2, nbatch=nbatch, scratch=scratch)


CASES = [
    _case("small_pm2_uniform", (64, 3, 3, 32, 64, 3), [KSMALL]),
    _case("small_flat_64x64", (8, 6, 6, 32, 64, 3), [KSMALL]),
    _case("small_128x32", (8, 6, 6, 32, 96, 3), [KSMALL]),
    _case("small_1x1_uniform", (1, 8, 8, 32, 64, 1), [KSMALL]),
    _case("small_1x1_bordered", (1, 8, 9, 32, 64, 1), [KSMALL]),
    _case("tiles_383_small", (383, 8, 16, 32, 64, 3), [KSMALL]),
    _case("tiles_384_128x64", (48, 32, 32, 32, 64, 3), [K64]),
    _case("t128x128", (48, 32, 32, 32, 128, 3), [K128]),
    _case("t128x32", (48, 32, 32, 32, 32, 3), [K32]),
    _case("rows_first_rule", (16384, 1, 1, 32, 128, 1), [KROWS]),
    _case("rows_first_rule_under", (16320, 1, 1, 32, 128, 1), [KSMALL]),
    _case("rows_second_rule", (24576, 1, 1, 32, 256, 1), [KROWS]),
    _case("rows_second_rule_under", (24448, 1, 1, 32, 256, 1), [KSMALL]),
    _case("pm_lds_dma", (640, 9, 9, 32, 96, 3), [K96]),
    _case("pm_lds_dma_res", (640, 9, 9, 32, 96, 3), [K96], res=True),
    _case("pm_lds_dma_x2", (640, 9, 9, 32, 96, 3), [K96], cin2=32),
    _case("n511_flat_128x96", (511, 10, 10, 32, 96, 3), [K96]),
    _case("row8_flat", (2, 21, 21, 4, 64, 7), [KROW8]),
    _case("row8_pixel_major", (512, 7, 7, 4, 64, 7), [KROW8]),
    _case("batched_small", (8, 6, 6, 32, 64, 3), [KSMALL], nbatch=3),
    _case("batched_large", (48, 32, 32, 32, 64, 3), [K64], nbatch=3),
    _case("splitk_12_chunk_rule", (64, 3, 3, 64, 64, 3), [KSMALL], scratch=8),       # S settles at 3: 36 chunks / 3 = 12
    _case("splitk_two_slices", (64, 3, 3, 64, 64, 3), [KSMALL], scratch=2),          # S = 2: the scratch holds no third slice
]
IDS = [c["key"] for c in CASES]


def _operands(c):
    """-> x [nbatch][n,h,w,cin], weight [nbatch][cout,cin_w,ks,ks], bias, x2, w2, res (float32 numpy; None where absent)"""
    n, h, w, cin, cout, ks = c["shape"]
    rng = np.random.default_rng(1900 + IDS.index(c["key"]))
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    nb, cin_w = c["nbatch"], (3 if ks == 7 else cin)
    x = f(nb, n, h, w, cin)
    if ks == 7:
        x[..., 3] = 0.0                                  # the NHWC4 staging: the fourth channel is padding
    wt = f(nb, cout, cin_w, ks, ks) * np.float32(np.sqrt(2.0 / (cin_w * ks * ks)))
    bias = f(cout) * np.float32(0.1)
    x2 = f(n, h, w, c["cin2"]) if c["cin2"] else None
    w2 = f(cout, c["cin2"], 1, 1) * np.float32(np.sqrt(2.0 / c["cin2"])) if c["cin2"] else None
    res = f(n, h, w, cout) if c["res"] else None
    return x, wt, bias, x2, w2, res


def run_case(native, c):
    """the launches' profile records and the digest of y, through the entry point the case belongs to"""
    n, h, w, cin, cout, ks = c["shape"]
    x, wt, bias, x2, w2, res = _operands(c)
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    xd, bd, x2d, resd = t(x), t(bias), t(x2), t(res)
    if c["cin2"]:
        pw, pb = native.conv_pack_fused2(t(wt[0]), bd, None, t(w2), None, None)
    else:
        packs = [native.conv_pack(t(wt[b]), bd) for b in range(c["nbatch"])]
        pw, pb = torch.stack([p[0] for p in packs]), packs[0][1]
    scratch = None
    if c["scratch"]:
        scratch = torch.empty(c["scratch"] * n * h * w * ((cout + 31) // 32 * 32), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    native.profile_enable(8)
    native.profile_reset()
    if c["cin2"]:
        y = native.conv_nhwc_fused2(xd[0], x2d, pw, pb, cout, ks, 1)
    elif c["nbatch"] > 1:
        y = torch.empty(c["nbatch"], n, h, w, cout, dtype=torch.float32, device=DEV)
        d = native.ConvDesc(n, h, w, cin, cout, ks, 1)
        native.check(native.lib().be_conv_nhwc_batched_f32(C.byref(d), native.dptr(xd), native.dptr(pw), native.dptr(pb), native.dptr(y), cout,
                                                           c["nbatch"], xd[0].numel(), pw[0].numel(), y[0].numel(),
                                                           native.stream_ptr(xd.device)), "be_conv_nhwc_batched_f32")
    else:
        y = native.conv_nhwc(xd[0], pw[0], pb, cout, ks, 1, residual=resd, scratch=scratch)
    torch.cuda.synchronize()
    recs = native.profile_read(8)
    native.profile_enable(0)
    yh = y.cpu().numpy()
    return {"launches": [[r[0], r[1], r[2], r[4]] for r in recs], "finite": bool(np.isfinite(yh).all()),
            "y": hashlib.sha256(np.ascontiguousarray(yh).tobytes()).hexdigest()}


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_convolution_takes_the_recorded_route_and_gives_the_recorded_bits(native, golden, c):
    got, want = run_case(native, c), golden[c["key"]]
    assert got["finite"]
    assert [l[0] for l in got["launches"]] == c["kernels"]           # the decision this case is here for
    assert got["launches"] == want["launches"]                       # kernel id, FLOPs, bytes, executed FLOPs of every launch
    assert got["y"] == want["y"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_conv_routes_gpu.py --record    (in the checkout whose library is to be recorded)")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "blurry-edges_amd"), os.path.join(ROOT, "tests")]
    from be_hip import native as n
    n.lib()
    cases = {c["key"]: run_case(n, c) for c in CASES}
    for c in CASES:
        assert cases[c["key"]]["finite"], c["key"]
        assert [l[0] for l in cases[c["key"]]["launches"]] == c["kernels"], (c["key"], cases[c["key"]]["launches"])
    with open(os.path.join(os.path.dirname(n.LIB_PATH), "BUILD_INFO.json")) as f:       # written by build() next to the library
        built = json.load(f)
    with open(GOLDEN, "w") as f:
        json.dump({"library_git_head": built.get("git_head"), "library_dirty": built.get("dirty"),
                   "cases": {k: {"launches": v["launches"], "y": v["y"]} for k, v in cases.items()}}, f, indent=1)
        f.write("\n")
    print(f"recorded {len(cases)} cases of {n.LIB_PATH} in {GOLDEN}")
