"""be_local_stage.hip's three plans on the CPU, through the host-only hooks: the region table of the packed buffer against the
offsets of the library before the table existed (tests/golden/local_stage_layout.json, derived from that library's own offset
arrays), the workspace size against that library's answers, and the route of a sub-batch against a table written out here, one
child interpreter per knob arm (the knobs are read once per process)."""
import json
import os
import subprocess
import sys

from conftest import ROOT

LAYOUT = os.path.join(ROOT, "tests", "golden", "local_stage_layout.json")
KNOBS = ("BE_WINO_NO_CHAIN", "BE_WINO_F32", "BE_ROWS_F32", "BE_L0_F32", "BE_C1_F32", "BE_NO_CONV_PM", "BE_NO_CONV1_POOL",
         "BE_WINO_NO_PERSIST", "BE_WINOGRAD", "BE_WINO_DS_GEMM")
# state_dict() order: (cout, cin, ksize); conv2 of a block at 2, 5, 8, 11 with its downsample behind it
LAYERS = [(64, 3, 7), (96, 64, 3), (96, 96, 3), (96, 64, 1), (256, 96, 3), (256, 256, 3), (256, 96, 1), (384, 256, 3), (384, 384, 3),
          (384, 256, 1), (256, 384, 3), (256, 256, 3), (256, 384, 1), (1024, 2304, 1), (10, 1024, 1)]


def _golden():
    with open(LAYOUT) as f:
        return json.load(f)


def test_region_table_tiles_the_packed_buffer_at_the_recorded_offsets():
    from be_hip import native
    lib = native.lib()
    regions, golden = native.local_stage_layout(), _golden()
    total = lib.be_local_stage_packed_floats()
    at = 0
    for k, r in enumerate(regions):                             # no gap, no overlap, in buffer order
        assert r["w_off"] == at and r["b_off"] == at + r["w_floats"] and r["w_off"] % 4 == 0, (k, r)
        assert r["w_floats"] + r["b_floats"] > 0, (k, r)
        at += r["w_floats"] + r["b_floats"]
        assert r["reads"] is None or 0 <= r["reads"] < k, (k, r)
    assert at == total == golden["total"]
    assert len({(r["layer"], r["form"]) for r in regions}) == len(regions)
    pad = lambda c: (c + 31) // 32 * 32
    for r in regions:                                           # each size is what the form's own sizing function says
        if r["form"] == "zero":
            assert (r["layer"], r["w_floats"], r["b_floats"], r["reads"]) == (-1, 0, 384, None)
            continue
        cout, cin, ks = LAYERS[r["layer"]]
        cin2 = LAYERS[r["layer"] + 1][1] if r["layer"] in (2, 5, 8, 11) else 0
        w, b, reads = {"f32": (lib.be_conv_packed_floats(cout, cin, ks), pad(cout), None),
                       "fused2": (lib.be_conv_fused2_packed_floats(cout, cin, ks, cin2), pad(cout), None),
                       "wino": (lib.be_wino_packed_floats(cout, cin), pad(cout), None),
                       "ds_f32": (lib.be_conv_packed_floats(cout, cin, 1), pad(cout), None),
                       "rows_bf6": (lib.be_gemm_rows_bf6_packed_floats(cout, cin), 0, (r["layer"], "f32" if r["layer"] == 13 else "ds_f32")),
                       "l0_bf6": (lib.be_conv3x3_pm_bf6_packed_floats(cout, cin, cin2), 0, (r["layer"], "fused2" if cin2 else "f32")),
                       "wino_ds": (lib.be_wino_ds_packed_floats(cout, cin), 0, None)}[r["form"]]
        assert w > 0 and (r["w_floats"], r["b_floats"]) == (w, b), r
        src = regions[r["reads"]] if r["reads"] is not None else None
        assert (src and (src["layer"], src["form"])) == reads, (r, src)
    forms = lambda layers, form: [r["layer"] for r in regions if r["form"] == form] == layers
    assert forms([0, 1, 4, 7, 10, 13, 14], "f32") and forms([2, 5, 8, 11], "fused2") and forms([4, 5, 7, 8, 10, 11], "wino")
    assert forms([6, 9, 12], "ds_f32") and forms([6, 9, 12, 13], "rows_bf6") and forms([1, 2], "l0_bf6") and forms([6, 9, 12], "wino_ds")
    assert regions == golden["regions"]                         # ... and every offset is the earlier library's


def test_workspace_bytes_are_the_recorded_ones():
    from be_hip import native
    lib = native.lib()
    want = _golden()["workspace_bytes"]
    assert len(want) == 21
    for n in (0, 1, 5, 8191, 8192, 8193, 20000):
        for chunk in (0, 2, 512):
            assert lib.be_local_stage_workspace_bytes(n, chunk) == want[f"{n},{chunk}"], (n, chunk)


# (staging, conv1, conv1_pools, l0_bf6, chain, blocks6, store_maps, fc1_bf6), native.LOCAL_STAGE_ROUTE_FIELDS.  staging: 1 = rows padded
# to 28 pixels; conv1: 0 k_conv_igemm, 1 pixel-major, 2 fp32 conv1 + pool, 3 split-bf16 conv1 + pool; blocks6: 0 direct, 1 Winograd
# with the downsample folded, 2 Winograd + split-bf16 downsample launch, 3 Winograd + fp32 downsample launch
_DIRECT_SMALL, _DIRECT_LARGE = (0, 0, 0, 0, 0, 0, 1, 0), (1, 2, 1, 0, 0, 0, 1, 0)
_DIRECT = [_DIRECT_SMALL, _DIRECT_SMALL, _DIRECT_LARGE]         # nb = 1, 511, 512: opts->winograd = 0 is the fp32 routing by size
_DEFAULT = (1, 3, 1, 1, 1, 1, 0, 1)                             # the Winograd path: one route at every sub-batch size
ROUTES = {                                                      # arm -> (environment, winograd = 0 routes, winograd = 1 routes)
    "default": ({}, _DIRECT, [_DEFAULT] * 3),
    "BE_WINO_F32=1": ({"BE_WINO_F32": "1"}, _DIRECT, [(0, 0, 0, 0, 1, 3, 1, 0), (0, 0, 0, 0, 1, 3, 1, 0), (1, 2, 1, 0, 1, 3, 1, 0)]),
    "BE_ROWS_F32=1": ({"BE_ROWS_F32": "1"}, _DIRECT, [(1, 3, 1, 1, 1, 3, 1, 0)] * 3),
    "BE_L0_F32=1": ({"BE_L0_F32": "1"}, _DIRECT, [(1, 3, 1, 0, 1, 1, 0, 1)] * 3),
    "BE_C1_F32=1": ({"BE_C1_F32": "1"}, _DIRECT, [(0, 0, 0, 1, 1, 1, 0, 1), (0, 0, 0, 1, 1, 1, 0, 1), (1, 2, 1, 1, 1, 1, 0, 1)]),
    "BE_WINO_DS_GEMM=1": ({"BE_WINO_DS_GEMM": "1"}, _DIRECT, [(1, 3, 1, 1, 1, 2, 1, 1)] * 3),
    "BE_WINO_NO_CHAIN=1": ({"BE_WINO_NO_CHAIN": "1"}, _DIRECT, [(1, 3, 1, 1, 0, 1, 1, 1)] * 3),
    "BE_WINO_NO_CHAIN=0": ({"BE_WINO_NO_CHAIN": "0"}, _DIRECT, [_DEFAULT] * 3),                    # set and 0: off
    "BE_NO_CONV_PM=0": ({"BE_NO_CONV_PM": "0"}, [_DIRECT_SMALL] * 3, [(0, 0, 0, 1, 1, 1, 0, 1)] * 3),    # set at all: on
    "BE_NO_CONV1_POOL=1": ({"BE_NO_CONV1_POOL": "1"}, [_DIRECT_SMALL, _DIRECT_SMALL, (1, 1, 0, 0, 0, 0, 1, 0)],
                           [(0, 0, 0, 1, 1, 1, 0, 1), (0, 0, 0, 1, 1, 1, 0, 1), (1, 1, 0, 1, 1, 1, 0, 1)]),
}

_ROUTE_CHILD = """
import json, sys
sys.path[:0] = {paths!r}
from be_hip import native
print(json.dumps([[[native.local_stage_route(w, nb)[f] for f in native.LOCAL_STAGE_ROUTE_FIELDS] for nb in (1, 511, 512)] for w in (0, 1)]))
"""


def test_route_of_a_sub_batch_in_every_knob_arm():
    from be_hip import native
    assert native.lib().be_local_stage_route_debug(1, 0, None) < 0                                  # refused, not answered
    for arm, (knobs, direct, wino) in ROUTES.items():
        env = dict(os.environ)
        for k in KNOBS:
            env.pop(k, None)
        env.update(knobs)
        r = subprocess.run([sys.executable, "-c", _ROUTE_CHILD.format(paths=[p for p in sys.path if p])], env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, (arm, r.stderr[-2000:])
        got = json.loads(r.stdout.splitlines()[-1])
        assert got == [[list(t) for t in direct], [list(t) for t in wino]], (arm, got)
