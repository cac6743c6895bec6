"""be_local_loss_f32 per patch and per term, in both launch variants, against the float64 reference of tests/loss_terms_oracle.py.

The entry point launches k_local_loss<WAVES> (a workgroup per patch) up to 1024 patches and k_local_loss<1> (a wave per patch, four
patch slots per workgroup, idle waves of the last workgroup shadowing the last patch) above.  One seeded set of 1031 patches serves
every case; a smaller case takes its first rows, so one reference (computed once) serves them all.

- partial [n,3] per patch and term: |delta| <= 1e-5 |ref| + 1e-6 max_patch |ref| (loss_terms_oracle.term_bound).
- the gradient under three weightings - (0, 0), the defaults, and a pair BALANCED from the reference so that the three weighted
  per-term gradients have the same L-inf norm (no chain can hide under another) - relmax(grad n 441, ref) <= 2e-4 each.
- position independence within a variant, want_grad on / off, run to run: bit for bit.
- the shadow waves store nothing (sentinel rows past n, a direct call of the C entry point).
- the extras of the large-batch kernel against the float64 composite (1e-5) and boundary map (5e-5).
- be_local_loss_finish_f32 against the float64 sum of the same partial: one float32 rounding, 2^-23.
A patch within 1e-6 of a branch threshold in the reference is left out of the per-patch comparisons: 1 of the 1031 (patch 268), so
1 of 1024 .. 1031 in the large cases and none in the cases of 1, 3 and 64 patches.

Worst observed error / bound on an MI355X (printed by the tests as `ratio ...` lines):
                                          k_local_loss<WAVES> (n 1 .. 1024)    k_local_loss<1> (n 1025 .. 1031)
  partial colour   (1e-5 rel + 1e-6 floor)             0.015                             0.011
  partial boundary (same)                              0.013                             0.012
  partial smoothness (same)                            0.030                             0.028
  gradient (0, 0)        / 2e-4                        0.012                             0.001
  gradient defaults      / 2e-4                        0.017                             0.001
  gradient balanced      / 2e-4                        0.028                             0.050
  extras patches / 1e-5, boundary / 5e-5                 -                            0.039, 0.001
  local_loss_finish / 2^-23: 0.38 at worst (B = 63); every case below half an ulp of the result.
The 1e-6 floor was not needed by any quantity: the worst boundary sum sits at 1.3 % of its bound, so the floor stays as the issue
set it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_terms_oracle as lt
from conftest import relmax

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = lt.LOCAL_SIZES_WORKGROUP + lt.LOCAL_SIZES_WAVE
DEFAULT_BETAS = (1e-3, 5e-4)
SENTINEL = 0x7FA5C3D2                                       # a NaN pattern no kernel arithmetic produces


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native
    import utils
    native.lib()
    helper = utils.PostProcessLocalBase(utils.get_args("local_train", argv=[]), DEV)
    inp = lt.local_inputs()
    return dict(native=native, opts=helper.render_opts(False), ref=lt.local_reference(**inp),
                inp={k: torch.from_numpy(v).to(DEV) for k, v in inp.items()}, runs={})


def f32(v):
    return float(np.float32(v))


def bits(t):
    return t.contiguous().view(torch.int32)


def launch(env, n, betas=DEFAULT_BETAS, want_grad=True, want=()):
    i = env["inp"]
    partial, grad, extra = env["native"].local_loss(env["opts"], i["est"][:n], i["img_fit"][:n], i["gt"][:n], i["bdist"][:n],
                                                    i["deri"][:n], betas[0], betas[1], want_grad=want_grad, want=want)
    torch.cuda.synchronize()
    return partial, grad, extra


def run(env, n, betas=DEFAULT_BETAS):
    """(partial, grad) of the ordinary call, once per (n, betas)"""
    key = (n, betas)
    if key not in env["runs"]:
        env["runs"][key] = launch(env, n, betas)[:2]
    return env["runs"][key]


def variant(n):
    return "k_local_loss<WAVES>" if n <= 1024 else "k_local_loss<1>"


@pytest.mark.parametrize("n", SIZES)
def test_partial_sums_per_patch_and_per_term(env, n):
    ref = env["ref"]["partial"][:n].numpy()
    got = run(env, n)[0].cpu().double().numpy()
    assert got.shape == (n, 3)
    keep = lt.kept_patches(env["ref"]["near"][:n])
    for k, name in enumerate(lt.LOCAL_TERMS):
        ratio = np.abs(got[:, k] - ref[:, k]) / lt.term_bound(ref[:, k])
        worst = int(keep[np.argmax(ratio[keep])])
        print(f"ratio partial {name} {variant(n)} n={n}: {ratio[worst]:.3f} at patch {worst} (ref {ref[worst, k]:.3e})")
        assert ratio[worst] <= 1.0, (name, worst, got[worst, k], ref[worst, k])


@pytest.mark.parametrize("weighting", ["colour_only", "defaults", "balanced"])
@pytest.mark.parametrize("n", SIZES)
def test_gradient_under_three_weightings(env, n, weighting):
    grads = [g[:n] for g in env["ref"]["grads"]]
    betas = {"colour_only": (0.0, 0.0), "defaults": (f32(DEFAULT_BETAS[0]), f32(DEFAULT_BETAS[1])),
             "balanced": lt.balanced_betas(grads)}[weighting]
    keep = lt.kept_patches(env["ref"]["near"][:n])
    got = run(env, n, betas)[1].cpu().double() * (n * 441)
    e = relmax(got[keep], lt.local_weighted_grad(grads, *betas)[keep])
    print(f"ratio grad {weighting} (beta_b {betas[0]:.4g}, beta_s {betas[1]:.4g}) {variant(n)} n={n}: {e / 2e-4:.3f}")
    assert e <= 2e-4


@pytest.mark.parametrize("big,small", [(1024, (1, 3, 64)), (1031, (1025, 1026, 1027))])
def test_a_patch_gives_the_same_bits_wherever_it_sits_in_the_launch(env, big, small):
    whole = run(env, big)[0]
    for n in small:
        assert torch.equal(bits(run(env, n)[0]), bits(whole[:n])), n


@pytest.mark.parametrize("n", [64, 1024, 1027, 1031])
def test_partial_is_bit_identical_without_the_gradient_and_run_to_run(env, n):
    partial, grad = run(env, n)
    p2, g2, _ = launch(env, n)
    assert torch.equal(bits(p2), bits(partial)) and torch.equal(bits(g2), bits(grad))
    p3, g3, _ = launch(env, n, want_grad=False)
    assert g3 is None and torch.equal(bits(p3), bits(partial))


def test_shadow_waves_of_the_last_workgroup_store_nothing(env):
    """n = 1025: the last workgroup has one live wave and three that shadow patch 1024.  Output buffers four patches longer than n,
    pre-filled with a sentinel: the rows past n keep it, the rows below equal the ordinary call's bits."""
    native, i, n, pad = env["native"], env["inp"], 1025, 4
    shapes = dict(partial=(3,), grad=(10,), patches=(3, 21, 21), boundary=(21, 21))
    buf = {k: torch.full((n + pad,) + s, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32) for k, s in shapes.items()}
    native.check(native.lib().be_local_loss_f32(C.byref(env["opts"]), *(native.dptr(i[k][:n]) for k in ("est", "img_fit", "gt", "bdist", "deri")),
                                                DEFAULT_BETAS[0], DEFAULT_BETAS[1], *(native.dptr(buf[k]) for k in shapes), n,
                                                native.stream_ptr(torch.device(DEV))), "be_local_loss_f32")
    torch.cuda.synchronize()
    partial, grad, extra = launch(env, n, want=("patches", "boundary"))
    plain = dict(partial=partial, grad=grad, **extra)
    for k in shapes:
        assert bool((bits(buf[k][n:]) == SENTINEL).all()), k
        assert torch.equal(bits(buf[k][:n]), bits(plain[k])), k
    assert torch.equal(bits(partial), bits(run(env, n)[0]))               # the call with extras and the one without: same sums


def test_extras_of_the_large_batch_kernel_vs_float64(env):
    n = 1031
    _, _, extra = launch(env, n, want=("patches", "boundary"))
    keep = lt.kept_patches(env["ref"]["near"][:n])
    e_p = relmax(extra["patches"].cpu()[keep], env["ref"]["patches"][keep])
    e_b = relmax(extra["boundary"].cpu()[keep], env["ref"]["boundary"][keep])
    print(f"ratio extras k_local_loss<1> n={n}: patches {e_p / 1e-5:.3f}  boundary {e_b / 5e-5:.3f}")
    assert e_p <= 1e-5 and e_b <= 5e-5


@pytest.mark.parametrize("B,betas", [(1, DEFAULT_BETAS), (63, DEFAULT_BETAS), (64, DEFAULT_BETAS), (65, DEFAULT_BETAS),
                                     (1031, DEFAULT_BETAS), (65, (0.3, 0.07)), (1031, (0.3, 0.07))])
def test_local_loss_finish_is_the_float64_sum_rounded_once(env, B, betas):
    """one wavefront, lane l takes patches l, l + 64, ..., then the DPP tree: B below, at and above a wavefront and far above"""
    partial = run(env, 1031)[0][:B].contiguous()
    got = float(env["native"].local_loss_finish(partial, betas[0], betas[1]).cpu())
    want = float(lt.local_loss_from_partial(partial, f32(betas[0]), f32(betas[1])))
    print(f"ratio finish B={B} betas={betas}: {abs(got - want) / abs(want) / 2.0 ** -23:.3f}")
    assert abs(got - want) <= 2.0 ** -23 * abs(want)
