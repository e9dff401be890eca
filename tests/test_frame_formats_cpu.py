"""Frame formats (BGR, NV12, YUYV frames in the input pipeline and the camera detector), the parts that need no GPU.

  - the Q16 integers of the "jfif" preset ARE libjpeg's decoder conversion: a JPEG decoded by Pillow to RGB equals, byte for byte, the
    same JPEG decoded to YCbCr (``draft``) and run through the restatement (tests/frame_formats_ref.py), at 4:4:4 and 4:2:0;
  - against Pillow's own YCbCr -> RGB ``convert`` (another fixed-point table) the restatement is within one code on all 2^24 triples;
  - the "bt709" integers are round(65536 x) of the published matrix, the restatement is within one code of the matrix in floating
    point on all triples, and no intermediate of either preset leaves int32;
  - the two new symbols: header block and top comment, library, ctypes table; ABI 5; lf_pipeline_plan_set_format's
    refusals and lf_pipeline_frame_bytes, on the host alone;
  - the package's presets are the restatement's; the Python-side validation of names, tuples and shapes;
  - no new instantiation of the two kernels spills or uses scratch, and the RGB instantiations keep their registers.
"""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest

import frame_formats_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = {"lf_pipeline_plan_set_format": 3, "lf_pipeline_frame_bytes": 1}          # name -> parameter count


def lib():
    from lanedetection_end2end_amd import _lib
    return _lib.load()


def preset(name):
    """the integers the PACKAGE ships (pipeline.YUV_PRESETS): the pins below are on them, not on the restatement's copy"""
    from lanedetection_end2end_amd import pipeline
    assert pipeline.YUV_PRESETS[name] == F.PRESETS[name]
    return pipeline.YUV_PRESETS[name]


def all_triples(chunk):
    """Y = 16 chunk .. 16 chunk + 15, every Cb, Cr: (16, 256, 256) uint8 arrays, 16 chunks cover the 2^24 triples"""
    Y, Cb, Cr = np.meshgrid(np.arange(16 * chunk, 16 * chunk + 16, dtype=np.uint8), np.arange(256, dtype=np.uint8),
                            np.arange(256, dtype=np.uint8), indexing="ij")
    return Y, Cb, Cr


@pytest.mark.parametrize("subsampling", [0, 2], ids=["444", "420"])
def test_jfif_integers_are_libjpegs_conversion(subsampling):
    from PIL import Image
    rng = np.random.default_rng(20 + subsampling)
    # smooth + noise: a JPEG of pure noise decodes to mid-grey mush; this one reaches saturated colours and both clamps
    base = rng.integers(0, 256, (12, 16, 3)).astype(np.float64)
    img = np.clip(np.kron(base, np.ones((8, 8, 1))) * 1.3 - 30 + rng.normal(0, 12, (96, 128, 3)), 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=92, subsampling=subsampling)
    rgb = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    im = Image.open(io.BytesIO(buf.getvalue()))
    im.draft("YCbCr", im.size)
    assert im.mode == "YCbCr"
    ycc = np.asarray(im)
    assert ycc.shape == (96, 128, 3) and rgb.shape == (96, 128, 3)
    mine = F.ycc_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2], preset("jfif"))
    assert (rgb == 0).any() and (rgb == 255).any(), "the image does not reach the clamps"
    differ = int((mine != rgb).sum())
    print("subsampling %d: %d of %d bytes differ" % (subsampling, differ, rgb.size))
    assert differ == 0


def test_jfif_within_one_code_of_pillows_convert():
    from PIL import Image
    worst, ones, total = 0, 0, 0
    jfif = preset("jfif")
    for chunk in range(16):
        Y, Cb, Cr = all_triples(chunk)
        ycc = np.stack([Y, Cb, Cr], axis=-1).reshape(16 * 256, 256, 3)
        pil = np.asarray(Image.frombytes("YCbCr", (256, 16 * 256), ycc.tobytes()).convert("RGB")).reshape(16, 256, 256, 3)
        d = np.abs(F.ycc_to_rgb(Y, Cb, Cr, jfif).astype(np.int16) - pil.astype(np.int16))
        worst, ones, total = max(worst, int(d.max())), ones + int((d == 1).sum()), total + d.size
    print("against Pillow's convert: max difference %d, %.1f %% of values differ by 1" % (worst, 100.0 * ones / total))
    assert worst == 1


def test_bt709_integers_and_int32():
    c_y, y_off, c_rv, c_gu, c_gv, c_bu = preset("bt709")
    matrix = (1.164384, 1.792741, 0.213249, 0.532909, 2.112402)
    assert (c_y, c_rv, c_gu, c_gv, c_bu) == tuple(int(round(x * 65536)) for x in matrix) and y_off == 16
    assert preset("jfif") == (65536, 0, 91881, 22554, 46802, 116130)
    worst = 0
    peak = {"jfif": 0, "bt709": 0}
    for chunk in range(16):
        Y, Cb, Cr = all_triples(chunk)
        mine, m = F.ycc_to_rgb(Y, Cb, Cr, F.PRESETS["bt709"], intermediates=True)
        peak["bt709"] = max(peak["bt709"], m)
        peak["jfif"] = max(peak["jfif"], F.ycc_to_rgb(Y, Cb, Cr, F.PRESETS["jfif"], intermediates=True)[1])
        ref = F.float_ycc_to_rgb(Y, Cb, Cr, matrix[0], 16, *matrix[1:])
        worst = max(worst, int(np.abs(mine.astype(np.int16) - ref.astype(np.int16)).max()))
    print("bt709 against the float matrix: max difference %d; largest intermediate %s" % (worst, peak))
    assert worst <= 1
    assert max(peak.values()) < 3.6e7 < 2 ** 31 - 1


def test_package_presets_are_the_restatements():
    from lanedetection_end2end_amd import pipeline
    assert pipeline.YUV_PRESETS == F.PRESETS and pipeline.PIXEL_FORMATS == F.FORMATS
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    assert "enum { LF_FRAME_RGB = 0, LF_FRAME_BGR = 1, LF_FRAME_NV12 = 2, LF_FRAME_YUYV = 3 };" in header
    for coef in F.PRESETS.values():
        assert "{%s}" % ", ".join(str(c) for c in coef) in header
    assert pipeline.yuv_coefficients("bt709") == F.PRESETS["bt709"] and pipeline.yuv_coefficients([1, 2, 3, 4, 5, 6]) == (1, 2, 3, 4, 5, 6)
    for bad in ("bt601", (1, 2, 3, 4, 5), (1, 2, 3, 4, 5, 6, 7), (1.0, 2, 3, 4, 5, 6), 7, None):
        with pytest.raises(ValueError, match="yuv"):
            pipeline.yuv_coefficients(bad)
    for fmt in F.FORMATS:
        assert pipeline.frames_shape(fmt, 2, (8, 6)) == F.frames_shape(fmt, 2, 8, 6)
    with pytest.raises(ValueError, match="pixel_format"):
        pipeline.frames_shape("rgba", 1, (8, 6))
    with pytest.raises(ValueError, match="even"):
        pipeline.frames_shape("nv12", 1, (7, 6))
    with pytest.raises(ValueError, match="even"):
        pipeline.frames_shape("nv12", 1, (8, 5))
    with pytest.raises(ValueError, match="even"):
        pipeline.frames_shape("yuyv", 1, (8, 5))
    assert pipeline.frames_shape("yuyv", 1, (7, 6)) == (1, 7, 6, 2)


def test_symbols_in_header_library_table_and_integration():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    top = header[:header.index("*/", header.index("#define LF_ABI_VERSION"))]
    m = re.search(r"additions since 5 \(frame formats\): ([^*]*)", top)
    assert m, "no 'additions since 5 (frame formats)' line"
    block = header[header.index("additions since 5 -- frame formats"):]
    sig = _lib._declare(lib())
    for name, nparams in SYMBOLS.items():
        assert name in m.group(1), name
        decl = re.search(r"^(int|size_t) %s\(([^;]*)\);" % name, block, re.M)
        assert decl, name
        assert len(decl.group(2).split(",")) == nparams == len(sig[name][1]), name
        assert hasattr(lib(), name) and name in _lib.exported_symbols(), name
        assert name in stub, name
    assert re.search(r"#define LF_ABI_VERSION 5\b", header) and lib().lf_abi_version() == 5


def test_set_format_and_frame_bytes_on_the_host():
    L = lib()
    Int6 = ctypes.c_int * 6
    jfif, bt709 = Int6(*F.PRESETS["jfif"]), Int6(*F.PRESETS["bt709"])

    def plan(H, W):
        p = ctypes.c_void_p(L.lf_pipeline_plan_create(H, W, 0, H, 4, 8))
        assert p, L.lf_last_error()
        return p

    p = plan(12, 20)
    try:
        assert L.lf_pipeline_frame_bytes(p) == 12 * 20 * 3                 # a plan that never gets the call: RGB
        for code, coef, want in ((1, None, 12 * 20 * 3), (2, jfif, 12 * 20 * 3 // 2), (3, bt709, 12 * 20 * 2), (2, None, 12 * 20 * 3 // 2),
                                 (0, None, 12 * 20 * 3)):
            assert L.lf_pipeline_plan_set_format(p, code, coef) == 0, L.lf_last_error()
            assert L.lf_pipeline_frame_bytes(p) == want == F.frame_bytes({v: k for k, v in F.FORMATS.items()}[code], 12, 20)
        for code in (-1, 4, 77):
            assert L.lf_pipeline_plan_set_format(p, code, jfif) != 0 and b"unknown format" in L.lf_last_error()
        assert L.lf_pipeline_frame_bytes(p) == 12 * 20 * 3                 # a refused call leaves the plan as it was
        # an intermediate could leave int32: refused
        assert L.lf_pipeline_plan_set_format(p, 2, Int6(1 << 24, 0, 1, 1, 1, 1)) != 0 and b"int32" in L.lf_last_error()
        assert L.lf_pipeline_plan_set_format(p, 3, Int6(65536, 0, 1 << 25, 1, 1, 1)) != 0
        assert L.lf_pipeline_plan_set_format(None, 1, None) != 0
        assert L.lf_pipeline_frame_bytes(None) == 0
    finally:
        L.lf_pipeline_plan_destroy(p)
    for H, W, code, ok in ((11, 20, 2, False), (12, 21, 2, False), (11, 21, 2, False), (11, 20, 3, True), (12, 21, 3, False),
                           (11, 21, 1, True), (11, 21, 0, True)):
        p = plan(H, W)
        try:
            rc = L.lf_pipeline_plan_set_format(p, code, jfif)
            assert (rc == 0) == ok, (H, W, code, L.lf_last_error())
            if not ok:
                assert b"even" in L.lf_last_error() and L.lf_pipeline_frame_bytes(p) == H * W * 3
        finally:
            L.lf_pipeline_plan_destroy(p)


def test_python_side_refusals_need_no_device():
    from lanedetection_end2end_amd.pipeline import InputPipeline
    with pytest.raises(ValueError, match="pixel_format"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format="i420")
    with pytest.raises(ValueError, match="yuv"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format="nv12", yuv="bt2020")
    with pytest.raises(ValueError, match="yuv"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format="nv12", yuv=(1, 2, 3))
    with pytest.raises(ValueError, match="even"):
        InputPipeline(8, "bp", frame_hw=(21, 32), crop=16, pixel_format="nv12")
    with pytest.raises(ValueError, match="even"):
        InputPipeline(8, "bp", frame_hw=(20, 33), crop=16, pixel_format="yuyv")
    with pytest.raises(ValueError, match="int32"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format="yuyv", yuv=(1 << 24, 0, 1, 1, 1, 1))
    for fmt in F.FORMATS:
        pipe = InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format=fmt, yuv="bt709")
        assert pipe.frames_shape == F.frames_shape(fmt, 1, 20, 32)[1:]
        assert lib().lf_pipeline_frame_bytes(pipe.handle) == F.frame_bytes(fmt, 20, 32)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_frame_stem.hip", "lf_pipeline.hip"], tmp_path_factory.mktemp("isa_frame_formats"))


def test_no_new_instantiation_spills(kernels):
    resize = [k for k in kernels if "resize_format_kernel" in k["mangled"]]
    stem = [k for k in kernels if "frame_format_stem_kernel" in k["mangled"]]
    # <KSX, KSY, FMT> and <KSX, KSY, T, FMT>: 7 / 7, 5 / 5 and the generic taps, fp32 and bf16 storage, formats 1 (bgr), 2 (nv12), 3 (yuyv)
    for taps in ("Li7ELi7E", "Li5ELi5E", "Li0ELi0E"):
        for fmt in (1, 2, 3):
            assert sum(("resize_format_kernelI%sLi%dEE" % (taps, fmt)) in k["mangled"] for k in resize) == 1, (taps, fmt)
            for t in ("f", "DF16b"):
                assert sum(("frame_format_stem_kernelI%s%sLi%dEE" % (taps, t, fmt)) in k["mangled"] for k in stem) == 1, (taps, t, fmt)
    assert len(resize) == 9 and len(stem) == 18
    for k in resize + stem:
        print("%-60s vgpr %3d agpr %3d lds %5d" % (k["mangled"][:60], k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, "two workgroups of 256 threads per SIMD set"
        assert k["lds"] == 0, "LDS is dynamic: the plan's bytes, the RGB layout for every format"


def test_rgb_instantiations_keep_their_registers(kernels):
    """(vgpr, agpr) of the commit before the formats: the RGB kernels are the code they were (DESIGN.md 4.6 has the table)."""
    want = {"resize_bilinear_kernel<0, 0>": (43, 0), "resize_bilinear_kernel<5, 5>": (28, 0), "resize_bilinear_kernel<7, 7>": (27, 0)}
    by_name = {k["name"]: k for k in kernels}
    for name, regs in want.items():
        k = by_name[name]
        assert (k["vgpr"], k["agpr"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"], k["lds"]) == regs + (0, 0, 0, 0), (name, k)
    rgb = [k for k in kernels if "17frame_stem_kernel" in k["mangled"]]
    assert len(rgb) == 6
    for k in rgb:
        assert (k["vgpr"], k["agpr"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"], k["lds"]) == (60, 4, 0, 0, 0, 0), k
