"""The float64 per-patch references of the loss-kernel tests (tests/loss_terms_oracle.py) and the conditions on those tests' inputs,
checked without a GPU: a broken reference or a lost branch shows here first.

- Summed and weighted, the per-patch references equal the trusted oracles (oracle.render.local_loss, oracle.global_loss.global_loss
  with G, Gd, Gb computed its way) to 1e-12 relative, term by term and in total.
- The seeded global inputs visit all four etas2depth branches, the three depth-mask values, an empty and a live mask count, and
  both signs of sg1 / sg2; no more than 1 % of any case's patches lie within 1e-6 of a branch threshold.
"""
import numpy as np
import pytest
import torch

import loss_terms_oracle as lt
from oracle import depth as odepth, global_loss as ogl, render as orr

TIE = 1e-12
GLOBAL_KEYS = ("est", "img_fit", "img_gt", "G", "Gd", "Gb", "bdist", "deri", "bdepth")


@pytest.fixture(scope="module")
def local_case():
    inp = lt.local_inputs()
    return inp, lt.local_reference(**inp)


@pytest.fixture(scope="module", params=list(lt.GLOBAL_CASES) + ["host"])
def global_case(request):
    B, H, W, stride = lt.GLOBAL_CASES.get(request.param, lt.HOST_CASE)
    inp = lt.global_inputs(B, H, W, stride, request.param)
    c = odepth.depth_consts()
    return c, inp, lt.global_reference(c, stride=stride, **{k: inp[k] for k in GLOBAL_KEYS})


def rel(a, b):
    a, b = float(torch.as_tensor(a).detach()), float(torch.as_tensor(b).detach())
    return abs(a - b) / abs(b)


@pytest.mark.parametrize("betas", [(1e-3, 5e-4), (0.0, 0.0), (0.3, 0.07)])
def test_local_reference_sums_to_the_local_loss_oracle(local_case, betas):
    inp, ref = local_case
    n = 257                                                   # the per-patch terms do not depend on the batch: any prefix will do
    args = [lt.D(inp[k][:n]) for k in ("est", "img_fit", "gt", "bdist", "deri")]
    args[0].requires_grad_(True)
    loss, patches, bnd = orr.local_loss(*args, beta_b=betas[0], beta_s=betas[1])
    assert rel(lt.local_loss_from_partial(ref["partial"][:n], *betas), loss) <= TIE
    grad = torch.autograd.grad(loss, args[0])[0]
    mine = lt.local_weighted_grad([g[:n] for g in ref["grads"]], *betas) / (n * 441)
    assert float((mine - grad).abs().max()) <= TIE * float(grad.abs().max())
    assert torch.equal(patches.detach(), ref["patches"][:n]) and torch.equal(bnd.detach(), ref["boundary"][:n])


def test_local_inputs_stay_inside_the_exclusion_cap_at_every_size(local_case):
    _, ref = local_case
    for n in lt.LOCAL_SIZES_WORKGROUP + lt.LOCAL_SIZES_WAVE:
        assert len(lt.kept_patches(ref["near"][:n])) >= n - n // 100          # kept_patches asserts the cap (below 100: none)
    b_b, b_s = lt.balanced_betas(ref["grads"])
    w = [float(g.abs().max()) * k for g, k in zip(ref["grads"], (1.0, b_b, b_s * 441.0 / 361.0))]
    assert max(w) / min(w) <= 1 + 1e-6                        # the balanced pair does balance the three chains


def test_global_reference_sums_to_the_global_loss_oracle(global_case):
    """with G, Gd, Gb folded from the same est (oracle.global_loss's way), every normalised term and the weighted loss"""
    c, inp, _ = global_case
    B, P, stride = inp["est"].shape[0], inp["est"].shape[1], inp["stride"]
    G, Gd, Gb = lt.folded_maps(inp["est"], inp["img_fit"], stride)
    ref = lt.global_reference(c, inp["est"], inp["img_fit"], inp["img_gt"], G, Gd, Gb, inp["bdist"], inp["deri"], inp["bdepth"], stride)
    est = lt.D(inp["est"]).requires_grad_(True)
    loss, terms = ogl.global_loss(c, est, *(lt.D(inp[k]) for k in ("img_fit", "img_gt", "bdist", "deri", "bdepth")),
                                  gamma=lt.GAMMA_DISTINCT7, stride=stride)
    mine, mterms = lt.global_loss_from_partial(ref["partial"], lt.GAMMA_DISTINCT7, B, P)
    assert rel(mine, loss) <= TIE
    for k in terms:
        assert rel(mterms[k], terms[k]) <= TIE, k
    # ... and the gradients: gamma_k / n_k on the six term gradients, gamma_depth / count on the depth numerator's
    grad = torch.autograd.grad(loss, est)[0]
    g = lt.GAMMA_DISTINCT7
    w = sum(g[k] / n * ref["grads"][i] for i, (k, n) in enumerate(zip(lt.GLOBAL_TERMS, lt.global_normalisers(B, P))))
    w[..., 8:12] += g["depth"] / ref["partial"][:, lt.COL_COUNT].sum() * ref["gdepth"].reshape(B, P, 4)
    assert float((w - grad).abs().max()) <= TIE * float(grad.abs().max())


def test_global_inputs_visit_every_branch_and_stay_clear_of_the_thresholds(global_case):
    _, inp, ref = global_case
    lt.check_branch_coverage(ref)
    assert len(lt.kept_patches(ref["near"])) >= ref["near"].numel() * (1 - lt.MAX_EXCLUDED)
    bd = inp["bdepth"]
    assert 0.4 <= float((bd != 0).mean()) <= 0.6              # bdepth: non-zero on roughly half the pixels
    for b in range(1, bd.shape[0]):                           # different data per image
        assert not np.array_equal(inp["img_gt"][b], inp["img_gt"][0]) and not np.array_equal(inp["est"][b], inp["est"][0])


def test_global_case_shapes_are_the_ones_that_tell_the_axes_apart():
    from oracle import tiling as ot
    grids = {k: ot.grid_dims(H, W, s) for k, (B, H, W, s) in lt.GLOBAL_CASES.items()}
    assert grids == {"b3_25x29_s2": (3, 5), "b2_27x24_s3": (3, 2)}
    for B, H, W, s in lt.GLOBAL_CASES.values():
        assert B > 1 and H != W
    assert {s for _, _, _, s in lt.GLOBAL_CASES.values()} == {2, 3}
