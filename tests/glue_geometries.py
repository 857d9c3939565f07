"""Geometries at which the glue kernels of csrc/elastic_kernels.hip leave their 4-elements-per-thread forms, and the launcher's
rule that decides it, restated on the CPU.

``ed_gather_views``, ``ed_pick_assemble``, ``ed_unpad_direction``, ``ed_assemble_rows`` (four instantiations <T, PX4, GX4> per dtype) and
``ed_assemble_rows_x`` take the 4-wide form of a part only if its padded width, its crop width and its left pad offset are all
multiples of 4 (and every pointer accessed 16 bytes at a time is 16-byte aligned):

    px4 = gPW % 4 == 0 and w  % 4 == 0 and g_off_x % 4 == 0      the pick ("global") rows
    gx4 = vPW % 4 == 0 and Sw % 4 == 0 and v_off_x % 4 == 0      the view rows

``launch_class`` computes (px4, gx4) from geometry.PickPlan / ViewPlan / PadPlan exactly as pipeline.py builds them for an image.
``ops.TIMER`` records entry points, not template instantiations, so a GPU run cannot tell which form ran: this restatement, asserted
by tests/test_glue_geometries.py, is the only check that the case tables of the GPU suite reach every class.  The geometric half
of the rule is all that is restated; the tables of the GPU tests allocate their tensors whole, which torch aligns to 16 bytes.

Not a conftest and not collected: shared tables and helpers only.
"""
import torch

# name -> (Hl, Wl, h, w, d): latent size, reduced size (geometry.reduced_size of the image), model size
SCALAR_GEOMETRIES = {
    "ff_one_view": (64, 38, 64, 38, 64),     # 512x304 px: V = 1, both parts padded to 64 wide at g_off_x = v_off_x = 13
    "ff_views": (96, 54, 64, 36, 64),        # 768x432 px: V = 3, Sw = 54 at v_off_x = 5, w = 36 at g_off_x = 14
    "ft": (65, 32, 64, 31, 64),              # 520x256 px: V = 3, w = 31 (odd), overlapping centre rows; views 4-wide
    "tf": (66, 34, 64, 32, 64),              # 528x272 px: V = 3, Sw = 34 at v_off_x = 15; picks 4-wide
    "ff_xl": (128, 75, 128, 75, 128),        # 1024x600 px (SDXL): V = 1, off_x = 26
    "ft_many": (240, 135, 64, 36, 64),       # 1920x1080 px portrait: V = 40, overlaps on both axes, g_off_x = 14
}
# the class the issue lists for each name; tests/test_glue_geometries.py holds the restated rule to it
EXPECTED_CLASS = {"ff_one_view": (False, False), "ff_views": (False, False), "ft": (False, True), "tf": (True, False),
                  "ff_xl": (False, False), "ft_many": (False, True)}
# image sizes (sd_version, model size, height px, width px) of the same geometries, for the end-to-end rows
SCALAR_IMAGES = {"ff_one_view": ("1.5", 64, 512, 304), "ff_views": ("1.5", 64, 768, 432), "ft": ("1.5", 64, 520, 256),
                 "tf": ("1.5", 64, 528, 272), "ff_xl": ("XL1.0", 128, 1024, 600), "ft_many": ("1.5", 64, 1920, 1080)}

VIEW_ROWS = [(Hl, Wl, d, None) for Hl, Wl, _, _, d in SCALAR_GEOMETRIES.values()]           # VIEW_CASES: Hl, Wl, sample, patch
PICK_ROWS = [(Hl, Wl, h, w) for Hl, Wl, h, w, _ in SCALAR_GEOMETRIES.values()]              # PICK_CASES: Hl, Wl, h, w
FUSED_ROWS = [(Hl, Wl, h, w, d, None) for Hl, Wl, h, w, d in SCALAR_GEOMETRIES.values()]    # FUSED_CASES: .., d, patch


def plans(Hl, Wl, h, w, d, patch=None):
    """(PickPlan, ViewPlan, pick PadPlan, view PadPlan) as ElasticDiffusion builds them for model size ``d`` (window = stride =
    ``patch`` or d // 2, context = d - window)."""
    from elasticdiffusion_official_amd import geometry
    ws = patch if patch is not None else d // 2
    pp, vp = geometry.PickPlan(Hl, Wl, h, w), geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    return pp, vp, geometry.PadPlan(h, w, d), geometry.PadPlan(vp.Sh, vp.Sw, d)


def pick_x4(h, w, d):
    """the launcher's px4 (ed_pick_assemble, ed_unpad_direction, the pick part of ed_assemble_rows[_x]) for whole, aligned tensors"""
    from elasticdiffusion_official_amd import geometry
    gpad = geometry.PadPlan(h, w, d)
    return gpad.PW % 4 == 0 and w % 4 == 0 and gpad.left % 4 == 0


def view_x4(Hl, Wl, d, patch=None):
    """the launcher's gx4 (ed_gather_views with the pad offsets, the view part of ed_assemble_rows[_x])"""
    from elasticdiffusion_official_amd import geometry
    ws = patch if patch is not None else d // 2
    vp = geometry.ViewPlan(Hl, Wl, ws, ws, d - ws)
    vpad = geometry.PadPlan(vp.Sh, vp.Sw, d)
    return vpad.PW % 4 == 0 and vp.Sw % 4 == 0 and vpad.left % 4 == 0


def crop_x4(Hl, Wl, d, patch=None):
    """the form of ed_gather_views WITHOUT pad offsets (rows of the crop's own size): 4-wide iff the crop width is"""
    from elasticdiffusion_official_amd import geometry
    ws = patch if patch is not None else d // 2
    return geometry.ViewPlan(Hl, Wl, ws, ws, d - ws).Sw % 4 == 0


def launch_class(Hl, Wl, h, w, d, patch=None):
    """(px4, gx4) of ed_assemble_rows / ed_assemble_rows_x for this geometry"""
    return pick_x4(h, w, d), view_x4(Hl, Wl, d, patch)


def pick_model_size(h, w):
    """the model size tests/test_hip_parity.py's pick test derives from a PICK_CASES row"""
    return 128 if max(h, w) > 64 else 64


def misaligned(t, device="cuda:0"):
    """a device copy of ``t`` that starts one element past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 != 0 and view.is_contiguous()
    return view
