"""LocalStage's eval path (be_local_stage.hip: the region table, the workspace plan, the route) held to the library from before
they were stated once: per knob arm one child process (the knobs are read once per process) packs synth's weights and runs the
forward over a few batches; the sha256 of the packed buffer and of each of its regions (tests/golden/local_stage_layout.json), the
sha256 of the logits and the profiler's kernel ids per launch must be those of tests/golden/local_stage_plan.json, recorded on the
MI355X with that earlier library by this file's own child.

A packed-buffer digest that differs while the digests of every other process agree is what profiles/HISTORY.md rounds 28-29
describe; the assertion names the differing regions."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "local_stage_plan.json")
LAYOUT = os.path.join(ROOT, "tests", "golden", "local_stage_layout.json")
DEV = "cuda:0"
KNOBS = ("BE_WINO_NO_CHAIN", "BE_WINO_F32", "BE_ROWS_F32", "BE_L0_F32", "BE_C1_F32", "BE_NO_CONV_PM", "BE_NO_CONV1_POOL",
         "BE_WINO_NO_PERSIST", "BE_WINOGRAD", "BE_WINO_DS_GEMM", "BE_LIB_DIR", "BE_TORCH_OPS")


def _flat(n, winograd=1, chunk=0):
    return dict(key=("" if winograd else "direct_") + f"n{n}" + (f"_c{chunk}" if chunk else ""), n=n, chunk=chunk, winograd=winograd, view=False)


# arm -> (environment, the packed buffer is digested, cases).  A patch's bits depend on neither batch nor chunk in the default arm, so
# few cases are needed there: one patch; 5 in sub-batches of 2, 2, 1 (the `first` offsets of input and output), flat and gathered
# from an image pair; 1024, where the Winograd buffers turn tile-major.  The fp32 routing changes kernels at 512 patches, and its
# downsample at 480 (the smallest batch the weight-stationary GEMM takes)
ARMS = {
    "default": ({}, True, [_flat(1), _flat(5, chunk=2), dict(_flat(5, chunk=2), key="view_n5_c2", view=True), _flat(1024),
                           _flat(3, 0), _flat(511, 0), _flat(512, 0)]),
    "BE_WINO_F32=1": ({"BE_WINO_F32": "1"}, True, [_flat(3), _flat(480), _flat(512), _flat(1024)]),
    "BE_ROWS_F32=1": ({"BE_ROWS_F32": "1"}, False, [_flat(3), _flat(480), _flat(512)]),
    "BE_C1_F32=1": ({"BE_C1_F32": "1"}, False, [_flat(3), _flat(512)]),
    "BE_L0_F32=1": ({"BE_L0_F32": "1"}, False, [_flat(3)]),
    "BE_WINO_DS_GEMM=1": ({"BE_WINO_DS_GEMM": "1"}, False, [_flat(3)]),
    "BE_WINO_NO_CHAIN=1": ({"BE_WINO_NO_CHAIN": "1"}, False, [_flat(3)]),
    "BE_NO_CONV1_POOL=1": ({"BE_NO_CONV1_POOL": "1"}, False, [_flat(512, 0)]),
    "BE_NO_CONV_PM=1": ({"BE_NO_CONV_PM": "1"}, False, [_flat(512, 0)]),
}


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def region_name(r):
    return f"layer{r['layer']}.{r['form']}" if r["layer"] >= 0 else r["form"]


def measure(arm):
    """In the child: -> {"packed": {"all": sha, "regions": {name: sha}} (where digested), "cases": {key: {"logits": sha,
    "kernels": [id per launch]}}}.  Weights from synth.local_stage_state_dict(), patches from synth.uniform_patches (hashed on the CPU)."""
    import models
    from be_hip import native, synth
    _, digest_pack, cases = ARMS[arm]
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    packed = native.local_stage_pack([t.detach() for t in m._tensor_list()], eps=m.conv1[1].eps)
    torch.cuda.synchronize()
    out = {"cases": {}}
    if digest_pack:
        with open(LAYOUT) as f:
            layout = json.load(f)
        p = packed.cpu().numpy()
        assert p.size == layout["total"], (p.size, layout["total"])
        out["packed"] = {"all": _sha(p), "regions": {region_name(r): _sha(p[r["w_off"]:r["b_off"] + r["b_floats"]]) for r in layout["regions"]}}
    x = torch.from_numpy(synth.uniform_patches(max(c["n"] for c in cases), name="local_stage_plan")).to(DEV)
    img = torch.from_numpy(synth.uniform_patches(3, name="local_stage_plan_image").reshape(-1)[:2 * 3 * 21 * 25].reshape(2, 3, 21, 25).copy()).to(DEV)
    native.profile_enable(256)
    for c in cases:
        native.profile_reset()
        if c["view"]:                                        # 3 patch positions per image: the 5 patches span both images
            view = native.view_image_pair(img, stride=2)
            y, _ = native.local_stage_forward_view(packed, view, 3, c["n"], img.device, winograd=bool(c["winograd"]), chunk=c["chunk"])
        else:
            y, _ = native.local_stage_forward(packed, x[:c["n"]].contiguous(), winograd=bool(c["winograd"]), chunk=c["chunk"])
        torch.cuda.synchronize()
        ids = [r[0] for r in native.profile_read(256)]
        y = y.cpu().numpy()
        assert y.shape == (c["n"], 10) and np.isfinite(y).all(), c["key"]
        out["cases"][c["key"]] = {"logits": _sha(y), "kernels": ids}
    native.profile_enable(0)
    return out


_CHILD = r'''
import json, os, sys
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_local_stage_plan_gpu as t
print("RESULT " + json.dumps(t.measure(os.environ["BE_ARM"])))
'''


def run_arm(arm):
    """One child process under the arm's knobs (every other knob stripped) -> measure(arm)"""
    env = dict(os.environ, BE_ROOT=ROOT, BE_ARM=arm)
    for k in KNOBS:
        env.pop(k, None)
    env.update(ARMS[arm][0])
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (arm, r.stdout[-2000:] + r.stderr[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


@pytest.mark.gpu
@pytest.mark.parametrize("arm", list(ARMS))
def test_pack_logits_and_launches_are_those_of_the_library_before_the_plan(arm):
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    with open(GOLDEN) as f:
        want = json.load(f)["arms"][arm]
    got = run_arm(arm)
    print(arm, json.dumps(got))
    assert sorted(got["cases"]) == sorted(want["cases"]) == sorted(c["key"] for c in ARMS[arm][2])
    if ARMS[arm][1]:
        differing = [name for name, sha in want["packed"]["regions"].items() if got["packed"]["regions"].get(name) != sha]
        assert not differing and got["packed"] == want["packed"], (arm, "packed regions that differ from the golden", differing)
    else:
        assert "packed" not in want and "packed" not in got
    for key, w in want["cases"].items():
        assert got["cases"][key]["kernels"] == w["kernels"], (arm, key, "launches", got["cases"][key]["kernels"], w["kernels"])
        assert got["cases"][key]["logits"] == w["logits"], (arm, key, "logits")
