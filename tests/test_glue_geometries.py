"""CPU: which form -- 4 elements per thread or scalar -- of each glue kernel the case tables of the GPU suite reach, by the
launcher's rule restated in tests/glue_geometries.py.  ``ops.TIMER`` names entry points, not template instantiations, so on the GPU a
table that has drifted back to all-4-wide sizes would still pass: this is the check that it has not."""
import pytest

from elasticdiffusion_official_amd import geometry
from tests import glue_geometries as G
from tests import test_hip_parity as P
from tests import test_inpaint9_gpu as I9

ALL_CLASSES = {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("name", list(G.SCALAR_GEOMETRIES))
def test_named_geometry_has_its_class(name):
    Hl, Wl, h, w, d = G.SCALAR_GEOMETRIES[name]
    assert G.launch_class(Hl, Wl, h, w, d) == G.EXPECTED_CLASS[name]
    assert G.EXPECTED_CLASS[name] != (True, True)
    # the image size of the end-to-end row is this geometry, through the pipeline's own reduction
    sd, d_img, H, W = G.SCALAR_IMAGES[name]
    assert (H // 8, W // 8, *geometry.reduced_size(H, W, sd), d_img) == (Hl, Wl, h, w, d)
    # the pick test derives its model size from (h, w)
    assert G.pick_model_size(h, w) == d


def test_geometry_notes_hold():
    """the offsets and view counts the table's comments state"""
    seen = {}
    for name, geo in G.SCALAR_GEOMETRIES.items():
        _, vp, gpad, vpad = G.plans(*geo)
        seen[name] = (vp.V, geo[3], gpad.left, vp.Sw, vpad.left)
    assert seen == {"ff_one_view": (1, 38, 13, 38, 13), "ff_views": (3, 36, 14, 54, 5), "ft": (3, 31, 16, 32, 16),
                    "tf": (3, 32, 16, 34, 15), "ff_xl": (1, 75, 26, 75, 26), "ft_many": (40, 36, 14, 64, 0)}, seen


def test_fused_tables_reach_all_four_classes():
    old = [c for c in P.FUSED_CASES if c not in G.FUSED_ROWS]
    assert len(old) + len(G.FUSED_ROWS) == len(P.FUSED_CASES)          # the named rows are in the table
    assert {G.launch_class(*c) for c in old} == {(True, True)}         # what the suite ran before them
    assert {G.launch_class(*c) for c in P.FUSED_CASES} == ALL_CLASSES  # ed_assemble_rows <T, PX4, GX4>, offsets of the epilogue
    rows_x = {G.launch_class(*geo) for geo in I9.GEOMETRIES.values()}
    assert rows_x == ALL_CLASSES, rows_x                               # ed_assemble_rows_x
    e2e = [row for row in _edge_rows() if row[:4] in G.SCALAR_IMAGES.values()]
    assert len(e2e) == len(G.SCALAR_IMAGES)                            # every named size runs end to end


def _edge_rows():
    mark = [m for m in P.test_edge_geometries_and_prompt_batches_vs_oracle.pytestmark if m.name == "parametrize"][0]
    return [tuple(r) for r in mark.args[1]]


def test_view_and_pick_tables_reach_the_scalar_kernels():
    views = {(G.crop_x4(Hl, Wl, d, patch), G.view_x4(Hl, Wl, d, patch)) for Hl, Wl, d, patch in P.VIEW_CASES}
    assert {v[0] for v in views} == {True, False} and {v[1] for v in views} == {True, False}, views   # ed_gather_views, both calls
    picks = {G.pick_x4(h, w, G.pick_model_size(h, w)) for _, _, h, w in P.PICK_CASES}
    assert picks == {True, False}                                      # ed_pick_assemble / ed_unpad_direction


def test_a_scalar_view_case_reads_its_frame():
    """at least one VIEW_CASES row is padded AND scalar, so gather_windows_body's frame branch is compared with plain slicing"""
    hits = []
    for Hl, Wl, d, patch in P.VIEW_CASES:
        ws = patch if patch is not None else d // 2
        vp = geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
        if geometry.PadPlan(vp.Sh, vp.Sw, d).padded and not G.view_x4(Hl, Wl, d, patch):
            hits.append((Hl, Wl))
    assert hits
