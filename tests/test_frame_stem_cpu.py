"""Camera frames in the frozen detector, the parts that need no GPU: the new symbols (header, library, ctypes table),
the plan's answer to "does the fused resize + stem kernel take this geometry" with its LDS bytes restated in numpy, and the ISA
metadata of csrc/lf_frame_stem.hip.

The staging of a source window is SHARED with resize_bilinear_kernel (csrc/lf_pipeline_dev.h), so the metadata of the existing
pipeline kernels must be what it was before the sharing; the stem's kernels are not touched (frame_stem_kernel keeps a labelled copy
of their tile arithmetic) and are pinned all the same.  The values of the commit before this feature, (vgpr, agpr, vgpr spill, sgpr
spill, scratch):
  resize_bilinear_kernel<0, 0>        (43, 0, 0, 0, 0)
  resize_bilinear_kernel<5, 5>        (28, 0, 0, 0, 0)
  resize_bilinear_kernel<7, 7>        (27, 0, 0, 0, 0)
  label_kernel                        (14, 0, 0, 0, 0)
  horizon_kernel                      (14, 0, 0, 0, 0)
  stem_fwd_kernel<3, float, true>     (60, 4, 0, 0, 0)
  stem_fwd_kernel<3, bf16, true>      (60, 4, 0, 0, 0)
  stem_fwd_kernel<3, float, false>    (64, 4, 0, 0, 0)
  stem_fwd_kernel<3, bf16, false>     (64, 4, 0, 0, 0)
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("lf_pipeline_frame_stem_ok", "lf_pipeline_frame_stem_lds_bytes", "lf_pipeline_frame_stem_tile",
           "lf_lane_infer_u8_workspace_bytes", "lf_lane_infer_seg_u8_workspace_bytes", "lf_lane_infer_folded_u8",
           "lf_lane_infer_seg_folded_u8")
LDS_BUDGET = 64 * 1024
TILES = ((4, 32), (2, 32), (4, 16))          # stem pixels per workgroup, in the order the plan tries them

# (Hin, Win, crop_top, crop_h, out_h, out_w) -> does the fused kernel take it
GEOMS = {
    (180, 320, 20, 160, 64, 128): 1, (100, 130, 20, 80, 64, 128): 1, (30, 50, 6, 24, 32, 64): 1, (97, 333, 33, 64, 36, 68): 1,
    (40, 60, 10, 30, 12, 20): 1, (8, 8, 0, 8, 2, 2): 1,
    (720, 1280, 80, 640, 256, 512): 1, (720, 1280, 80, 640, 320, 640): 1, (720, 1280, 80, 640, 512, 1024): 1,
    (640, 1280, 0, 640, 64, 128): 0,              # 21 taps per axis: the source window of the smallest tile is > 100 KB
    (720, 1280, 80, 640, 64, 128): 0,
    (8, 8, 0, 8, 3, 2): 0, (8, 8, 0, 8, 2, 3): 0,   # the stem needs an even image
}

PARENT = {
    "resize_bilinear_kernel<0, 0>": (43, 0, 0, 0, 0), "resize_bilinear_kernel<5, 5>": (28, 0, 0, 0, 0),
    "resize_bilinear_kernel<7, 7>": (27, 0, 0, 0, 0), "label_kernel": (14, 0, 0, 0, 0), "horizon_kernel": (14, 0, 0, 0, 0),
}
PARENT_STEM = {          # by mangled name: the demangler at hand does not know the __bf16 instantiation's type code
    "_ZN12_GLOBAL__N_115stem_fwd_kernelILi3EfLb1EEEvPKfiiiS2_S2_PT0_PfiS2_S2_": (60, 4, 0, 0, 0),
    "_ZN12_GLOBAL__N_115stem_fwd_kernelILi3EDF16bLb1EEEvPKfiiiS2_S2_PT0_PfiS2_S2_": (60, 4, 0, 0, 0),
    "_ZN12_GLOBAL__N_115stem_fwd_kernelILi3EfLb0EEEvPKfiiiS2_S2_PT0_PfiS2_S2_": (64, 4, 0, 0, 0),
    "_ZN12_GLOBAL__N_115stem_fwd_kernelILi3EDF16bLb0EEEvPKfiiiS2_S2_PT0_PfiS2_S2_": (64, 4, 0, 0, 0),
}


def lib():
    from lanedetection_end2end_amd import _lib
    return _lib.load()


def test_symbols_in_header_library_table_and_integration():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    table = _lib.exported_symbols()
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
        assert hasattr(lib(), name) and name in table, name
        assert name in stub, name
    assert "LF_INFER_FRAME_TWO_LAUNCH = 2" in header and "LF_INFER_THIN = 1" in header
    debug = open(os.path.join(ROOT, "lanedetection_end2end_amd", "csrc", "lf_debug.h")).read()
    assert re.search(r"^int lf_debug_frame_stem\(", debug, re.M) and hasattr(lib(), "lf_debug_frame_stem")
    assert "lf_debug_frame_stem" in table and "lf_debug_frame_stem" not in header


def test_abi_is_still_5_and_both_lines_are_there():
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    assert re.search(r"#define LF_ABI_VERSION 5\b", header) and lib().lf_abi_version() == 5
    top = header[:header.index("*/", header.index("#define LF_ABI_VERSION"))]
    assert re.search(r"additions since 5 \(frozen --clas heads\): lf_convchain_infer_fold, lf_convchain_infer_folded,\s+"
                     r"lf_clas_tail_workspace_bytes, lf_clas_tail", top)
    m = re.search(r"additions since 5 \(camera frames\): ([^*]*)", top)
    assert m, "no 'additions since 5 (camera frames)' line"
    for name in SYMBOLS:
        assert name in m.group(1), name
    assert "additions since 5 -- camera frames" in header


def host_tables(plan, oh, ow):
    ksx, ksy = ctypes.c_int(), ctypes.c_int()
    assert lib().lf_pipeline_tables_host(plan, ctypes.byref(ksx), ctypes.byref(ksy), None, None, None, None, None, None) == 0
    arrs = [np.zeros(n, dtype=np.int32) for n in (2 * ow, ow * ksx.value, 2 * oh, oh * ksy.value)]
    ptrs = [a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
    assert lib().lf_pipeline_tables_host(plan, None, None, *ptrs, None, None) == 0
    return arrs[0].reshape(-1, 2), arrs[2].reshape(-1, 2), ksx.value, ksy.value


def window(bounds, out, tile):
    """largest source extent of the 2 t + 1 resized pixels a tile of t stem pixels reads (the pixel before the tile is the padding
    at the first tile)"""
    n = 0
    for o in range(0, out // 2, tile):
        a, b = max(0, 2 * o - 1), 2 * min(o + tile, out // 2) - 1
        n = max(n, int(bounds[b, 0] + bounds[b, 1] - bounds[a, 0]))
    return n


def restated_lds(bx, by, ksx, ksy, oh, ow):
    if oh % 2 or ow % 2:
        return 0, (0, 0)
    for th, tw in TILES:
        rows, cols = window(by, oh, th), window(bx, ow, tw)
        in_stride = (cols * 3 + 3 + ksx * 3 + 3) // 4 * 4           # [shift <= 3][window][over-read of up to ksx taps], dwords
        h_stride = ((2 * tw + 1) * 3 + 3) // 4 * 4
        shift = ((rows + 1) * 4 + 15) // 16 * 16
        bytes_h = shift + (rows + 1) * in_stride                      # staged source rows (+ one spare)
        fp32_at = (bytes_h + (rows + ksy) * h_stride + 15) // 16 * 16  # horizontal pass rows (+ the taps' over-read)
        total = fp32_at + 3 * (2 * th + 1) * (2 * tw + 2) * 4          # resized window: 3 planes, even / odd columns apart
        if total <= LDS_BUDGET:
            return total, (th, tw)
    return 0, (0, 0)


@pytest.mark.parametrize("geom", sorted(GEOMS), ids=lambda g: "%dx%d+%d+%d-%dx%d" % g)
def test_plan_reports_whether_the_geometry_fits(geom):
    L = lib()
    plan = ctypes.c_void_p(L.lf_pipeline_plan_create(*geom))
    assert plan, L.lf_last_error()
    try:
        ok = L.lf_pipeline_frame_stem_ok(plan)
        assert ok == GEOMS[geom]
        th, tw = ctypes.c_int(-1), ctypes.c_int(-1)
        assert L.lf_pipeline_frame_stem_tile(plan, ctypes.byref(th), ctypes.byref(tw)) == 0
        bx, by, ksx, ksy = host_tables(plan, geom[4], geom[5])
        want, tile = restated_lds(bx, by, ksx, ksy, geom[4], geom[5])
        got = L.lf_pipeline_frame_stem_lds_bytes(plan)
        print(geom, "ok", ok, "tile", (th.value, tw.value), "LDS bytes", got)
        assert got == want and (th.value, tw.value) == tile and got <= LDS_BUDGET
        assert (got > 0) == bool(ok)
        if ok:
            assert th.value * tw.value // 16 >= 4, "a whole 16-pixel MFMA tile per wave"
    finally:
        L.lf_pipeline_plan_destroy(plan)
    assert L.lf_pipeline_frame_stem_ok(None) == 0 and L.lf_pipeline_frame_stem_lds_bytes(None) == 0


def test_u8_workspace_is_the_fp32_one_plus_the_image_slot():
    L = lib()
    plan = ctypes.c_void_p(L.lf_erfnet_plan_create(2, 64, 128, 3, 2, 1))
    try:
        slot = 2 * 3 * 64 * 128 * 4
        for mode in (0, 2, 3):
            base = L.lf_lane_infer_workspace_bytes(plan, mode, 2, 2)
            assert base and L.lf_lane_infer_u8_workspace_bytes(plan, mode, 2, 2) == base + slot
            base = L.lf_lane_infer_seg_workspace_bytes(plan, mode, 2, 2)
            assert base and L.lf_lane_infer_seg_u8_workspace_bytes(plan, mode, 2, 2) == base + slot
        assert L.lf_lane_infer_u8_workspace_bytes(plan, 1, 2, 2) == 0 and L.lf_lane_infer_u8_workspace_bytes(plan, 0, 3, 2) == 0
        assert L.lf_lane_infer_seg_u8_workspace_bytes(plan, 0, 5, 2) == 0
    finally:
        L.lf_erfnet_plan_destroy(plan)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_frame_stem.hip", "lf_pipeline.hip", "lf_stem.hip"], tmp_path_factory.mktemp("isa_frame_stem"))


def test_frame_stem_kernels_do_not_spill(kernels):
    mine = [k for k in kernels if "frame_stem_kernel" in k["mangled"]]
    # <KSX, KSY, T>: 7 / 7, 5 / 5 and the generic taps, fp32 and bf16 storage
    for taps in ("Li7ELi7E", "Li5ELi5E", "Li0ELi0E"):
        assert sum(("frame_stem_kernelI%sfE" % taps) in k["mangled"] for k in mine) == 1, taps
        assert sum(("frame_stem_kernelI%sDF16bE" % taps) in k["mangled"] for k in mine) == 1, taps
    assert len(mine) == 6
    for k in mine:
        print("%-90s vgpr %3d agpr %3d lds %5d" % (k["mangled"], k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, "two workgroups of 256 threads per SIMD set"
        # static LDS + the largest dynamic size the plan may ask for stays inside the budget
        assert k["lds"] + LDS_BUDGET <= LDS_BUDGET, k


def test_existing_pipeline_and_stem_kernels_are_as_before(kernels):
    by_name = {k["name"]: k for k in kernels}
    by_mangled = {k["mangled"]: k for k in kernels}
    for table, found in ((PARENT, by_name), (PARENT_STEM, by_mangled)):
        for name, want in table.items():
            k = found[name]
            assert (k["vgpr"], k["agpr"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"]) == want, (name, k)
