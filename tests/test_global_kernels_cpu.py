"""The bounds test_global_kernels_gpu.py holds the GlobalStage kernels to are reachable by the reference arithmetic alone: for every
attention and LayerNorm case of that file the oracle's plain float32 evaluation is compared with its float64 evaluation on the same
inputs, per (batch, head) or per row, and must stay within HALF of the bound the GPU test uses.  Also: head_err itself, the slice rule
the cases rely on, and that the planted score spikes do leave the fast path in exactly one key slice.
"""
import numpy as np
import pytest
import torch

import global_kernels_oracle as gk


def test_head_err_sees_a_small_head_that_a_whole_tensor_norm_hides():
    B, L, H = 2, 64, 3
    ref = torch.from_numpy(gk.synth.hash_uniform(1, "gk_head_err", (B * L, H * 16))) * 2 - 1
    ref = ref / ref.abs().max()                                          # the tensor's maximum is 1
    blk = ref.view(B, L, H, 16)
    blk[1, :, 2] *= 0.1 / blk[1, :, 2].abs().max()                       # one head with max|ref| = 0.1 of it
    got = ref.clone()
    got.view(B, L, H, 16)[1, 17, 2, 5] += 1e-4
    e = gk.head_err(got, ref, B, L, H)
    assert e.shape == (B, H) and abs(float(e[1, 2]) - 1e-3) < 1e-9
    assert float(e.sum()) == float(e[1, 2])                              # and only that head
    assert abs(gk.relmax(got, ref) - 1e-4) < 1e-12                       # a whole-tensor norm reports a tenth of it ...
    got = ref.clone()
    got.view(B, L, H, 16)[1, 17, 2, 5] += 1e-5                           # ... so 1e-5 in that head reads 1e-4 per head, 1e-5 overall
    assert abs(float(gk.head_err(got, ref, B, L, H)[1, 2]) - 1e-4) < 1e-9 and abs(gk.relmax(got, ref) - 1e-5) < 1e-12
    assert float(gk.head_err(got, ref, B, L, H, rows=17).max()) == 0.0   # rows past the limit are not compared
    r = gk.row_err(got.view(B * L, -1), ref.view(B * L, -1))
    assert int((r > 0).sum()) == 1 and int(r.argmax()) == L + 17


def test_the_cases_sit_where_the_slice_rule_changes():
    assert [c.nz for c in gk.SLICE_CASES] == [4, 2, 1, 1]
    assert [(c.L // 128) * c.B * c.H for c in gk.SLICE_CASES] == [32, 288, 512, 30]
    assert gk.expected_nz(1, 8, 4096) == 4 and gk.expected_nz(2, 8, 4096) == 1         # one 147x147 pair: 256 workgroups; two: 512
    assert all(c.nz == 4 for c in gk.RAGGED_CASES + gk.SPIKE_CASES)
    widths = {c.name: [b - a for a, b in gk.slice_blocks(c.L, c.l_valid, c.nz)] for c in gk.RAGGED_CASES}
    assert widths["ragged_2048_lv1921"] == [15, 15, 15, 16] and widths["ragged_2048_lv1952"] == [15, 15, 15, 16]
    assert widths["ragged_2048_lv1953"] == [15, 16, 15, 16] and widths["ragged_2048_lv2047"] == [16, 16, 16, 16]
    assert widths["ragged_2176_lv2049"] == [16, 16, 16, 17] and widths["ragged_2176_lv2080"] == [16, 16, 16, 17]
    assert widths["ragged_2176_lv2081"] == [16, 17, 16, 17] and widths["ragged_2176_lv2175"] == [17, 17, 17, 17]
    for c in gk.INFER_CASES + [gk.InferCase("t", B, H, L) for B, H, L, _, _ in gk.TRAIN_CASES]:
        assert c.B * c.H * c.L <= 65536


@pytest.mark.parametrize("case", gk.SPIKE_CASES, ids=repr)
def test_the_planted_spike_leaves_the_fast_path_in_one_slice_only(case):
    hot = gk.SPIKE_SLICE[case.name]
    for bh in range(case.B * case.H):
        rise = gk.slice_rise(case, bh)                                   # [nz, L]
        share = (rise > 60).float().mean(dim=1)
        print(f"{case.name} head {bh}: share of rows above 60 binades per slice {share.tolist()}, largest rise {float(rise.max()):.0f}")
        assert float(share[hot]) > 0.5
        assert all(float(share[z]) == 0.0 for z in range(case.nz) if z != hot)


@pytest.mark.parametrize("case", gk.INFER_CASES, ids=repr)
def test_attention_float32_reference_reaches_half_the_bound(case):
    o64, l64 = case.ref(torch.float64)
    o32, l32 = case.ref(torch.float32)
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64
    eo = gk.head_err(o32, o64, case.B, case.L, case.H, rows=case.rows)
    el = gk.row_err(l32, l64, cols=case.rows)
    print(f"\nfloat32 vs float64 {case.name}: out worst head {float(eo.max()):.2e} (bound {case.bound():.0e})  lse {float(el.max()):.2e}")
    assert float(eo.max()) <= 0.5 * case.bound()
    assert float(el.max()) <= 0.5 * gk.BOUNDS["lse"]
    assert bool(torch.isfinite(o64).all())


@pytest.mark.parametrize("case", gk.TRAIN_CASES, ids=gk.train_name)
def test_training_attention_float32_autograd_reaches_half_the_bound(case):
    B, H, L, p, lv = case
    name = gk.train_name(case)
    qkv, dout = gk.make_qkv(name, B, L, H), gk.make_dout(name, B, L, H, lv)
    mask = gk.attention_keep(B, L, H, p, gk.TRAIN_SEED) if p > 0 else None
    if p > 0:
        per_head = mask.view(B * H, -1).mean(dim=1)
        assert float((per_head - (1 - p)).abs().max()) < 4e-3            # 410k draws per head: sigma 5e-4
    o64, l64, g64 = gk.train_ref(qkv, dout, B, L, H, p, lv, mask, torch.float64)
    o32, l32, g32 = gk.train_ref(qkv, dout, B, L, H, p, lv, mask, torch.float32)
    rows, D = (L if lv is None else lv), H * 16
    eo = float(gk.head_err(o32, o64, B, L, H, rows=rows).max())
    el = float(gk.row_err(l32, l64, cols=rows).max())
    eg = [float(gk.head_err(g32[:, i * D:(i + 1) * D], g64[:, i * D:(i + 1) * D], B, L, H, rows=rows).max()) for i in range(3)]
    print(f"\nfloat32 vs float64 {name}: out {eo:.2e}  lse {el:.2e}  dq {eg[0]:.2e}  dk {eg[1]:.2e}  dv {eg[2]:.2e}")
    assert eo <= 0.5 * gk.out_bound(name) and el <= 0.5 * gk.BOUNDS["lse"] and max(eg) <= 0.5 * gk.BOUNDS["grad"]
    if lv is not None:
        assert float(g64.view(B, L, -1)[:, lv:].abs().max()) == 0.0       # the padding rows take no gradient


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("D", gk.LN_D_CASES)
def test_layernorm_float32_reference_reaches_half_the_bound(D, with_res):
    for rows in gk.LN_ROWS_CASES:
        x, res, gamma, beta, _ = gk.ln_inputs(rows, D)
        res = res if with_res else None
        v64, y64 = gk.layernorm_ref(x, res, gamma, beta, dtype=torch.float64)
        _, y32 = gk.layernorm_ref(x, res, gamma, beta, dtype=torch.float32)
        ratio = gk.row_err(y32, y64) / gk.ln_row_bound(v64, y64, gamma, D)
        print(f"float32 vs float64 add_layernorm rows {rows} D {D} res {int(with_res)}: worst row error / bound {float(ratio.max()):.3f}"
              f" (row {int(ratio.argmax())})")
        assert float(ratio.max()) <= 0.5
        assert float(v64[rows - 1].var(unbiased=False)) == 0.0            # the constant row: eps alone decides
        assert torch.equal(y64[rows - 1], beta.double())
        if rows >= 2:
            assert abs(float(v64[0].mean()) - 1e4) < 1.0 and 0.5 < float(v64[0].std()) < 2.0


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_training_layernorm_float32_autograd_reaches_half_the_bound(p):
    for rows in gk.LN_TRAIN_ROWS:
        x, res, gamma, beta, dy = gk.ln_inputs(rows, 128, "lnt", plant=False)
        mask = gk.dropout_keep(rows * 128, p, 77, 5).view(rows, 128)
        got = {}
        for dt in (torch.float64, torch.float32):
            leaves = [t.to(dt).requires_grad_(True) for t in (x, res, gamma, beta)]
            _, y = gk.layernorm_ref(*leaves, mask=mask, p=p, dtype=dt)
            (y * dy.to(dt)).sum().backward()
            got[dt] = [y.detach()] + [t.grad for t in leaves]
        a, b = got[torch.float32], got[torch.float64]
        ey, edx, edv = (float(gk.row_err(a[i], b[i]).max()) for i in range(3))
        edg, edb = gk.relmax(a[3], b[3]), gk.relmax(a[4], b[4])
        print(f"float32 vs float64 layernorm_train rows {rows} p {p}: y {ey:.2e} dx {edx:.2e} dv {edv:.2e} dgamma {edg:.2e} dbeta {edb:.2e}")
        assert ey <= 0.5 * gk.BOUNDS["out"] and max(edx, edv, edg, edb) <= 0.5 * gk.BOUNDS["grad"]


def test_add_pe_reference_in_float32_is_one_rounding_per_element():
    for batches, per in gk.PE_CASES:
        x = torch.from_numpy(gk.synth.hash_normal(34, f"gk_pe_x_{batches}_{per}", (batches * per,)).astype(np.float32))
        pe = torch.from_numpy(gk.synth.hash_normal(35, f"gk_pe_{per}", (per,)).astype(np.float32))
        y32, y64 = gk.add_pe_ref(x, pe, batches, torch.float32), gk.add_pe_ref(x, pe, batches, torch.float64)
        assert torch.equal(y32, y64.float())                              # float32 add = the exact sum rounded once
