"""Checks of tests/train_layers_oracle.py, the float64 reference and the bounds of test_train_layers_gpu.py (no GPU needed):
the reference agrees with oracle.local_stage, the class-A bound passes torch's float32 evaluation with a factor two to spare at every
shape the GPU tests use, and it flags every planted defect of a kernel-like float32 implementation."""
import pytest
import torch
import torch.nn.functional as F

import train_layers_oracle as tl
from oracle import local_stage as ols

F32, F64 = torch.float32, torch.float64


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_reference_unit_equals_the_oracle_residual_block_in_float64():
    """the helper's conv + BatchNorm (+ res) + Smish stages chained into a residual block = oracle.local_stage.residual_block in
    train mode, and its running statistics = F.batch_norm's, to 1e-12"""
    n, h, w, cin, cout = 4, 5, 7, 32, 64
    a, b, c = (tl.conv_inputs(s, n, h, w, ci, cout, ks) for s, ci, ks in ((1, cin, 3), (2, cout, 3), (3, cin, 1)))
    sd = {}
    for name, d in (("conv1", a), ("conv2", b), ("downsample", c)):
        sd.update({f"blk.{name}.0.weight": d["w"].double(), f"blk.{name}.0.bias": d["b"].double(), f"blk.{name}.1.weight": d["gamma"].double(),
                   f"blk.{name}.1.bias": d["beta"].double(), f"blk.{name}.1.running_mean": torch.zeros(cout, dtype=F64),
                   f"blk.{name}.1.running_var": torch.ones(cout, dtype=F64)})

    def unit(x, d, ks, res=None, act=True):
        y = tl.conv_fwd(x, d["w"], d["b"], ks)
        st = tl.bn_stats(y, torch.zeros(cout), torch.ones(cout), eps=ols.BN_EPS, momentum=ols.BN_MOMENTUM)
        z = tl.bn_apply(y, st["mean"], st["invstd"], d["gamma"], d["beta"], res)
        return (tl.smish_fwd(z) if act else z), y, st

    x = a["x"].double()
    t, y1, st1 = unit(x, a, 3)
    ds_, _, _ = unit(x, c, 1, act=False)
    out, _, _ = unit(t, b, 3, res=ds_)
    want = ols.residual_block(tl.nchw(x), sd, "blk", training=True)
    assert relmax(tl.nchw(out), want) <= 1e-12
    assert relmax(tl.nchw(y1), F.conv2d(tl.nchw(x), a["w"].double(), a["b"].double(), padding=1)) <= 1e-12
    rm, rv = torch.zeros(cout, dtype=F64), torch.ones(cout, dtype=F64)
    F.batch_norm(tl.nchw(y1), rm, rv, None, None, True, ols.BN_MOMENTUM, ols.BN_EPS)
    assert relmax(st1["run_mean"], rm) <= 1e-12 and relmax(st1["run_var"], rv) <= 1e-12


def test_unit_cases_reach_the_launch_paths_they_are_listed_for():
    for name, c in tl.UNIT_CASES.items():
        assert tl.expected_path(c["shape"], c["chw"], c["want_dx"]) == c["path"], name
    paths = {c["path"] for c in tl.UNIT_CASES.values()}
    assert {p[1] for p in paths} == {"flat64", "pm64", "flat128", "pm128", "balanced", "conv1_mfma"}
    assert {p[2] for p in paths} == {"merged_v0", "merged_v1", "merged_v2", "balanced", "wgrad_alone", "conv1"}
    for key in ("res", "act", "dx_add", "want_dx"):                 # every switch on and off somewhere
        assert {c[key] for c in tl.UNIT_CASES.values()} == {True, False}, key
    # the split weight-gradient case: two slices, the last ragged - and no smaller M has more than one slice
    assert tl.wgrad_slices(1, 3, 11, 4, 4, 3) == (2, 32, 1)
    assert all(tl.wgrad_slices(1, 1, m, 4, 4, 3)[0] == 1 for m in range(1, 33))
    # be_linear_param_grads_f32 at 600 rows: S = min(512 / tiles, M / 256) = 2 slices of ceil16(300) = 304 and 296 rows
    assert (600 + 1) // 2 + (-((600 + 1) // 2) % 16) == 304


def _conv_cases():
    seen = {}
    for n, h, w, cin, cout, ks, chw in tl.WGRAD_CASES:
        seen[(n, h, w, cin, cout, ks, chw)] = ("wgrad",)
    for c in tl.UNIT_CASES.values():
        kinds = ("conv_fwd", "wgrad") + (("dgrad",) if c["want_dx"] else ())
        seen[c["shape"] + (c["chw"],)] = tuple(sorted(set(seen.get(c["shape"] + (c["chw"],), ()) + kinds)))
    for n, h, w, cin, cout in tl.PAIR_CASES.values():
        for ks in (3, 1):
            seen[(n, h, w, cin, cout, ks, 0)] = ("conv_fwd", "dgrad", "wgrad")
    return sorted(seen.items())


@pytest.mark.parametrize("case,kinds", _conv_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) and isinstance(v[0], int) else None)
def test_float32_torch_sits_inside_half_the_contraction_bound_at_every_gpu_shape(case, kinds):
    n, h, w, cin, cout, ks, chw = case
    if ks != 7 and cin % 32 and "conv_fwd" in kinds:
        pytest.fail("a unit needs cin % 32 == 0")
    d = tl.conv_inputs(100 + n + h + cin, n, h, w, cin, cout, ks, want_add=True)
    worst = {}
    if "conv_fwd" in kinds:
        worst["y"] = tl.worst(tl.ratio_a(tl.conv_fwd(d["x"], d["w"], d["b"], ks, chw, F32), tl.conv_fwd_ref(d["x"], d["w"], d["b"], ks, chw)))
    if "wgrad" in kinds:
        r = tl.wgrad_ref(d["x"], d["dy"], ks, chw)
        worst["dW"] = tl.worst(tl.ratio_a(tl.wgrad(d["x"], d["dy"], ks, chw, F32), r))
        assert bool((r["ref"][r["K"] == 0] == 0).all())              # taps that are never inside: reference exactly 0
    if "dgrad" in kinds:
        worst["dx"] = tl.worst(tl.ratio_a(tl.dgrad(d["dy"], d["w"], ks, chw, d["dx_add"], F32), tl.dgrad_ref(d["dy"], d["w"], ks, chw, d["dx_add"])))
    worst["db"] = tl.worst(tl.ratio_a(tl.col_sum(d["dy"], F32), tl.col_sum_ref(d["dy"])))
    print("ratio float32-cpu", case, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


@pytest.mark.parametrize("M,C", tl.BN_CASES)
def test_float32_torch_column_sums_sit_inside_half_the_bound(M, C):
    d = tl.bn_inputs(7, M, C)
    st = tl.bn_stats(d["y"], d["rm"], d["rv"])
    mean, invstd = st["mean"].float(), st["invstd"].float()
    worst = dict(col_sum=tl.worst(tl.ratio_a(tl.col_sum(d["y"], F32), tl.col_sum_ref(d["y"]))),
                 dbeta=tl.worst(tl.ratio_a(tl.col_sum(d["dout"], F32), tl.col_sum_ref(d["dout"]))),
                 dgamma=tl.worst(tl.ratio_a(tl.dgamma(d["dout"], d["y"], mean, invstd, F32), tl.dgamma_ref(d["dout"], d["y"], mean, invstd))))
    print("ratio float32-cpu", (M, C), {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst
    # the input set does what it is there for: a one-pass float32 variance (E[y^2] - E[y]^2) of the offset channels is far outside class B
    y32 = d["y"]
    one_pass = 1.0 / torch.sqrt(((y32 * y32).mean(0) - y32.mean(0) ** 2).clamp_min(0) + tl.BN_EPS)
    ref64, ref32 = tl.bn_stats(d["y"], d["rm"], d["rv"])["invstd"], tl.bn_stats(d["y"], d["rm"], d["rv"], F32)["invstd"]
    if M > 2:
        assert float(tl.ratio_b(one_pass, ref64, ref32).max()) > 1.0


def _linear_inputs(M, K, J, seed=5):
    g = tl.gen(seed)
    return tl.normal(g, M, K), tl.normal(g, J, K, scale=K ** -0.5), tl.normal(g, J, scale=0.1), tl.normal(g, M, J)


@pytest.mark.parametrize("M,K,J", tl.LINEAR_SMALL_CASES + tl.LINEAR_GRAD_CASES)
def test_float32_torch_linears_sit_inside_half_the_bound(M, K, J):
    x, w, b, dy = _linear_inputs(M, K, J)
    refs = tl.linear_bwd_ref(x, w, dy)
    got = dict(zip(("dx", "dw", "db"), tl.linear_bwd(x, w, dy, F32)))
    worst = {k: tl.worst(tl.ratio_a(got[k], refs[k])) for k in refs}
    worst["y"] = tl.worst(tl.ratio_a(tl.linear_fwd(x, w, b, F32), tl.linear_fwd_ref(x, w, b)))
    print("ratio float32-cpu", (M, K, J), {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5, worst


RECT = (3, 5, 7, 32, 32, 3, 0)            # the rectangular unit shape: every geometric defect shows on it
FC1 = (5, 1, 1, 72, 32, 1, 9)


def _kernel_like_ratio(kind, case, defect):
    n, h, w, cin, cout, ks, chw = case
    d = tl.conv_inputs(31, n, h, w, cin, cout, ks)
    got = tl.kernel_like(kind, d, ks, chw, defect)
    ref = {"conv_fwd": lambda: tl.conv_fwd_ref(d["x"], d["w"], d["b"], ks, chw), "wgrad": lambda: tl.wgrad_ref(d["x"], d["dy"], ks, chw),
           "dgrad": lambda: tl.dgrad_ref(d["dy"], d["w"], ks, chw)}[kind]()
    return tl.ratio_a(got, ref)


@pytest.mark.parametrize("kind", ["conv_fwd", "wgrad", "dgrad"])
@pytest.mark.parametrize("case", [RECT, FC1, (4, 2, 2, 32, 32, 3, 0)], ids=["rect", "fc1", "2x2"])
def test_the_kernel_like_float32_implementation_without_a_defect_passes(kind, case):
    assert tl.worst(_kernel_like_ratio(kind, case, None)) <= 0.5


@pytest.mark.parametrize("kind", ["conv_fwd", "wgrad", "dgrad"])
@pytest.mark.parametrize("defect", ["drop_row", "double_row", "wrong_neighbour", "swap_hw", "zero_column"])
def test_planted_defects_of_the_convolution_contractions_are_flagged(kind, defect):
    ratio = _kernel_like_ratio(kind, RECT, defect)
    bad = int((ratio > 1.0).sum())
    print(f"defect {defect} in {kind}: {bad} of {ratio.numel()} elements above the bound, worst {tl.worst(ratio):.3g}")
    assert bad >= 1


@pytest.mark.parametrize("kind", ["conv_fwd", "wgrad", "dgrad"])
def test_fc1_columns_in_hwc_order_are_flagged(kind):
    ratio = _kernel_like_ratio(kind, FC1, "hwc_columns")
    print(f"defect hwc_columns in {kind}: {int((ratio > 1.0).sum())} of {ratio.numel()} elements above the bound")
    assert int((ratio > 1.0).sum()) >= 1


@pytest.mark.parametrize("defect", ["drop_row", "double_row", "zero_column"])
def test_planted_defects_of_the_column_sums_and_linears_are_flagged(defect):
    """the contractions without a map (no tap, no h / w): K row dropped, doubled at a slice boundary, ragged last column left at zero"""
    d = tl.bn_inputs(7, 105, 100)
    st = tl.bn_stats(d["y"], d["rm"], d["rv"])
    xh = tl.xhat(d["y"], st["mean"].float(), st["invstd"].float(), F32)
    ones = torch.ones(105, 1)
    x, w, b, dy = _linear_inputs(64, 1024, 10)
    stats = (st["mean"].float(), st["invstd"].float())
    lin = tl.linear_bwd_ref(x, w, dy)
    # name -> (P [K, I], Q [K, J], K row at a slice boundary, what is added, take row 0, reference)
    cases = {"col_sum": (ones, d["dout"], 32, None, True, tl.col_sum_ref(d["dout"])),
             "dgamma": (ones, d["dout"] * xh, 32, None, True, tl.dgamma_ref(d["dout"], d["y"], *stats)),
             "linear_y": (x.t().contiguous(), w.t().contiguous(), 32, b, False, tl.linear_fwd_ref(x, w, b)),
             "linear_dx": (dy.t().contiguous(), w, 8, None, False, lin["dx"]),
             "linear_dw": (dy, x, 32, None, False, lin["dw"]),
             "linear_db": (torch.ones(64, 1), dy, 32, None, True, lin["db"])}
    for name, (P, Q, row, add, first, ref) in cases.items():
        def run(defect_):
            out = tl.gemm_kt(P, Q, defect_, row)
            out = out if add is None else out + add
            return tl.ratio_a(out[0] if first else out, ref)
        assert tl.worst(run(None)) <= 0.5, name
        assert int((run(defect) > 1.0).sum()) >= 1, (name, defect)


@pytest.mark.parametrize("kind", ["perm", "negative"])
def test_every_window_of_the_max_pool_inputs_has_a_unique_maximum(kind):
    for h, w, k, s, p in tl.POOL_CASES:
        for c in tl.POOL_CHANNELS:
            x = tl.pool_input(3, tl.POOL_N, h, w, c, kind)
            assert tl.pool_unique_max(x, k, s, p), (h, w, k, c)
            assert bool((x == x.round()).all()) and float(x.abs().max()) < 2 ** 20
            if kind == "negative":
                assert float(x.max()) < 0
    assert not tl.pool_unique_max(tl.pool_input(3, 3, 11, 11, 4, "ties"), 3, 2, 1)


def test_smish_extremes_are_planted_and_class_b_has_its_floor():
    row = tl.plant_smish(torch.zeros(3, 16))
    assert set(row.tolist()) == set(tl.SMISH_PLANT)
    ref = torch.tensor([[1.0, -2.0], [3.0, 0.5]], dtype=F64)
    r = tl.ratio_b(ref.float() + torch.tensor([[0.0, 0.0], [3 * tl.U * 3, 0.0]]), ref, ref.float())       # float32 run exact: the floor decides
    assert 0.5 < float(r[0]) <= 1.0 and float(r[1]) == 0.0
