"""Accuracy of split-bf16 (bf16x6) products in the Winograd transform-domain GEMMs, emulated on the CPU (numpy; nothing in the
product uses it).  The go / no-go of the bf16x6 GEMMs (be_wino.hip, k_wino_gemm_ps).

Each fp32 operand is split x = hi + mid + lo (bf16 pieces, round-to-nearest-even from what is left: exact for finite x whose lo stays
a bf16 normal); a product is the six bf16 MFMAs lo.hi, hi.lo, mid.mid, mid.hi, hi.mid, hi.hi per 16-deep K chunk, each MFMA adding the
exact sum of its 16 bf16 products to the fp32 accumulator with one rounding (bf16 x bf16 is exact in fp32; the sum is emulated in
float64).  The fp32 GEMM it replaces is an fmaf chain over K (v_mfma_f32_32x32x2_f32 is that chain bit for bit).  Both are measured
against the float64 GEMM on the six LocalStage layer shapes (K = cin), L-inf / L-inf, for three kinds of operands:
  random    normal activations, He-scaled weights
  trained   heavy-tailed (Student t, 3 dof) activations and weights: the outliers a trained network has
  stressed  the weights' rows and the activations' columns scaled over 1e-3 .. 1e3 (BatchNorm folds with extreme running_var)
Measured (this script, 256 rows): fp32 3.0-7.6e-7, bf16x6 1.4-5.5e-7 relative per GEMM - bf16x6 is 0.33-0.83x the fp32 error
(6 roundings per 16-deep chunk against 16; the dropped pieces are <= 3 x 2^-24 relative per product).  The Winograd layer error of
5-10e-6 (tests: 1.5e-5 bound) is the transforms' and the output transform's cancellation, which both arithmetics share; on the GPU
the six layer shapes measure the same for both (tests/test_wino_split_bf16.py).  Go: far below the ~1.2e-5 per-layer no-go line.
Round 9: the same two emulations at the four row-GEMM shapes of LocalStage's eval path (the 1x1 downsamples of layers 1-3, fc.1),
which run on the same kernel.  Measured (this script, 64 rows): bf16x6 0.51-0.75x the fp32 error on random operands (K = 2304: 1.1e-6
against 2.2e-6), worst ratio of the twelve cases 1.18 (heavy-tailed, K = 96: 1.6e-7 against 1.4e-7), every bf16x6 figure <= 1.1e-6.
    python lab/wino_split_bf16_error.py [rows]
"""
import sys

import numpy as np

LAYERS = [(96, 256), (256, 256), (256, 384), (384, 384), (384, 256), (256, 256)]
ROW_GEMMS = [(96, 256), (256, 384), (384, 256), (2304, 1024)]      # downsamples of layers 1-3, fc.1 (be::gemm_rows_bf6)


def bf16_rne(x):
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def split3(x):
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    return hi, mid, bf16_rne((r - mid).astype(np.float32))


def gemm_fp32(a, b):
    """fmaf chain over k: acc = fp32(a[:, k] b[k, :] + acc) (the product is exact in float64, the add rounds once to fp32)."""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for k in range(a.shape[1]):
        acc = (np.outer(a64[:, k], b64[k]) + acc).astype(np.float32)
    return acc


def gemm_bf16x6(a, b):
    pa, pb = [p.astype(np.float64) for p in split3(a)], [p.astype(np.float64) for p in split3(b)]
    order = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]       # lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k0 in range(0, a.shape[1], 16):
        for i, j in order:
            acc = (pa[i][:, k0:k0 + 16] @ pb[j][k0:k0 + 16] + acc).astype(np.float32)
    return acc


def operands(kind, rows, k, n, rng):
    if kind == "random":
        a, b = rng.standard_normal((rows, k)), rng.standard_normal((k, n)) * np.sqrt(2.0 / k)
    elif kind == "trained":
        a, b = rng.standard_t(3, (rows, k)), rng.standard_t(3, (k, n)) * np.sqrt(2.0 / k)
    else:
        a = rng.standard_normal((rows, k)) * 10.0 ** rng.uniform(-3, 3, (1, k))
        b = rng.standard_normal((k, n)) * 10.0 ** rng.uniform(-3, 3, (1, n)) * np.sqrt(2.0 / k)
    return a.astype(np.float32), b.astype(np.float32)


def relmax(x, ref):
    return float(np.abs(x.astype(np.float64) - ref).max() / np.abs(ref).max())


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    rng = np.random.default_rng(2026)
    worst = 0.0
    for kind in ("random", "trained", "stressed"):
        for cin, cout in LAYERS:
            a, b = operands(kind, rows, cin, cout, rng)
            ref = a.astype(np.float64) @ b.astype(np.float64)
            e32, e6 = relmax(gemm_fp32(a, b), ref), relmax(gemm_bf16x6(a, b), ref)
            worst = max(worst, e6)
            print(f"{kind:8s} K={cin:3d} N={cout:3d}: fp32 {e32:.2e}  bf16x6 {e6:.2e}  ratio {e6 / e32:.2f}")
    print(f"worst bf16x6 GEMM error {worst:.2e} ({'go' if worst <= 1.2e-5 else 'NO-GO'}: per-layer line 1.2e-5)")
    worst_ratio = 0.0
    for kind in ("random", "trained", "stressed"):
        for cin, cout in ROW_GEMMS:
            a, b = operands(kind, min(rows, 128), cin, cout, rng)
            ref = a.astype(np.float64) @ b.astype(np.float64)
            e32, e6 = relmax(gemm_fp32(a, b), ref), relmax(gemm_bf16x6(a, b), ref)
            worst_ratio = max(worst_ratio, e6 / e32)
            print(f"row GEMM {kind:8s} K={cin:4d} N={cout:4d}: fp32 {e32:.2e}  bf16x6 {e6:.2e}  ratio {e6 / e32:.2f}")
    print(f"row GEMMs: worst bf16x6 / fp32 error ratio {worst_ratio:.2f}")


if __name__ == "__main__":
    main()
