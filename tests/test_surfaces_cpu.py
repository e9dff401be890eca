"""Decoder surfaces (pitch, plane offsets, frame stride, plane pointers, I420, RGBX / BGRX), the parts that need no GPU.

  - tests/surface_ref.py: extract(embed(x)) == x for every format and layout, the padding really differs between seeds;
  - FrameLayout's arithmetic against hand-computed values (the decoder layout 1280 x 720 NV12, pitch 1536, chroma at row 736) and
    against the C side (lf_pipeline_surface_span, lf_pipeline_frame_bytes) and the restatement;
  - every refusal, on the Python side (ValueError, no device) and the C side (rc != 0, lf_last_error, the plan as it was);
  - the new symbols: header block and top comment, library, ctypes table, export list; ABI 5;
  - ISA metadata of the new kernels: no spills, no scratch, vgpr + agpr <= 128, static LDS 0;
  - the stand-alone host program (tests/surface_stage_host.cpp): the staging's address arithmetic over heap buffers of exactly
    batch_bytes / span(p) bytes, every load's extent asserted, against a per-pixel loop -- built with the address and
    undefined-behaviour sanitizers where the host compiler links them, and without.
"""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import frame_formats_ref as F
import surface_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = {"lf_pipeline_plan_set_layout": 3, "lf_pipeline_surface_span": 2}          # name -> parameter count
GEOMS = [(98, 334), (30, 50), (8, 8), (180, 320)]


def lib():
    from lanedetection_end2end_amd import _lib
    return _lib.load()


def tight_frames(fmt, N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, S.tight_shape(fmt, N, H, W), dtype=np.uint8)


@pytest.mark.parametrize("fmt", sorted(S.FORMATS))
def test_extract_inverts_embed(fmt):
    for H, W in GEOMS:
        x = tight_frames(fmt, 3, H, W, 11)
        for kind in (1, 2, 3, 4):
            L = S.kernel_layout(fmt, H, W, kind)
            batch, planes = S.embed(x, L, 5)
            assert batch.shape == (L.batch_bytes(3),) and all(planes[n][p].shape == (L.span[p],) for n in range(3) for p in range(len(L.dims)))
            assert np.array_equal(S.extract(batch, L, 3), x) and np.array_equal(S.extract(planes, L, 3), x)
            other, _ = S.embed(x, L, 6)
            assert np.array_equal(S.extract(other, L, 3), x) and not np.array_equal(other, batch), "the padding is seeded"
        tight = S.Layout(fmt, H, W)
        assert np.array_equal(S.embed(x, tight, 1)[0], x.reshape(-1)), "the layout of all defaults is the tight frame"


def test_to_rgb_of_the_new_formats():
    H, W = 6, 8
    x = tight_frames("i420", 2, H, W, 3)
    rgb = S.to_rgb(x, "i420", H, W, F.PRESETS["bt709"])
    Y, Cb, Cr = S.planes_of(x, "i420", H, W)
    for (n, y, xx) in ((0, 0, 0), (1, 5, 7), (0, 3, 2), (1, 2, 5)):
        want = F.ycc_to_rgb(Y[n, y, xx:xx + 1], Cb[n, y >> 1, (xx >> 1):(xx >> 1) + 1], Cr[n, y >> 1, (xx >> 1):(xx >> 1) + 1], F.PRESETS["bt709"])[0]
        assert tuple(rgb[n, y, xx]) == tuple(want)
    q = tight_frames("rgbx", 2, H, W, 4)
    assert np.array_equal(S.to_rgb(q, "rgbx", H, W), q[..., :3]) and np.array_equal(S.to_rgb(q, "bgrx", H, W)[..., 0], q[..., 2])
    assert np.array_equal(S.swap_chroma(S.swap_chroma(x, H, W), H, W), x)


def test_frame_layout_arithmetic():
    from lanedetection_end2end_amd.pipeline import FrameLayout, SURFACE_FORMATS, PIXEL_FORMATS
    assert SURFACE_FORMATS == S.FORMATS and PIXEL_FORMATS == F.FORMATS
    # what a hardware decoder writes: 1280 x 720 NV12, pitch 1536, the chroma plane behind 736 rows
    dec = FrameLayout("nv12", (720, 1280), pitch=(1536, 1536), plane_offsets=(0, 736 * 1536))
    assert (dec.planes, dec.plane_rows, dec.plane_row_bytes) == (2, (720, 360), (1280, 1280))
    assert dec.pitch == (1536, 1536) and dec.plane_offsets == (0, 1130496)
    assert dec.span == (719 * 1536 + 1280, 359 * 1536 + 1280) == (1105664, 552704)
    assert dec.frame_span == 736 * 1536 + 359 * 1536 + 1280 == 1683200
    assert dec.frame_stride == 736 * 1536 + 360 * 1536 == 1683456
    assert dec.batch_bytes(1) == 1683200 and dec.batch_bytes(4) == 3 * 1683456 + 1683200
    # one int is plane 0's pitch; later planes stay tight and follow directly
    a = FrameLayout("nv12", (8, 12), pitch=16)
    assert a.pitch == (16, 12) and a.plane_offsets == (0, 128) and a.span == (7 * 16 + 12, 3 * 12 + 12) and a.frame_stride == 128 + 48
    i = FrameLayout("i420", (8, 12), pitch=(15, 7, 9), frame_stride=1000)
    assert i.planes == 3 and i.plane_rows == (8, 4, 4) and i.plane_row_bytes == (12, 6, 6)
    assert i.plane_offsets == (0, 120, 148) and i.span == (117, 27, 33) and i.frame_span == 181 and i.frame_stride == 1000
    assert i.batch_bytes(3) == 2181
    # YV12: the offsets of planes 1 and 2 exchanged; the furthest plane is then plane 1
    yv = FrameLayout("i420", (8, 12), plane_offsets=(0, 120, 96))
    assert yv.plane_offsets == (0, 120, 96) and yv.frame_span == 120 + 24 and yv.frame_stride == 144
    x = FrameLayout("bgrx", (5, 7), pitch=32)
    assert x.plane_row_bytes == (28,) and x.span == (4 * 32 + 28,) and x.frame_stride == 160
    for fmt in S.FORMATS:
        t = FrameLayout(fmt, (8, 12))
        assert t.batch_bytes(3) == 3 * t.frame_stride == int(np.prod(S.tight_shape(fmt, 3, 8, 12)))
        for H, W in GEOMS:
            for kind in (1, 2, 3, 4):
                R = S.kernel_layout(fmt, H, W, kind)
                L = FrameLayout(fmt, (H, W), R.given[0], R.given[1], R.given[2], plane_pointers=R.pointers)
                assert (list(L.pitch), list(L.plane_offsets), list(L.span), L.frame_span, L.frame_stride, L.batch_bytes(3)) == \
                    (R.pitch, R.offsets, R.span, R.frame_span, R.stride, R.batch_bytes(3)), (fmt, H, W, kind)


REFUSED = [  # (format, (H, W), pitch, offsets, stride, a word of the reason)
    ("nv12", (7, 8), None, None, None, "even"), ("nv12", (8, 7), None, None, None, "even"), ("i420", (7, 8), None, None, None, "even"),
    ("i420", (8, 7), None, None, None, "even"), ("yuyv", (8, 7), None, None, None, "even"),
    ("rgb", (8, 8), 23, None, None, "below"), ("nv12", (8, 8), (8, 6), None, None, "below"), ("i420", (8, 8), (8, 4, 3), None, None, "below"),
    ("rgbx", (8, 8), 31, None, None, "below"),
    ("rgb", (8, 8), -24, None, None, "negative"), ("nv12", (8, 8), None, (0, -64), None, "negative"), ("bgr", (8, 8), None, None, -1, "negative"),
    ("nv12", (8, 8), None, (8, 64), None, "[0]"), ("rgb", (8, 8), None, (4,), None, "[0]"),
    ("yuyv", (8, 8), 18, None, None, "4"), ("rgbx", (8, 8), 34, None, None, "4"), ("bgrx", (8, 8), 33, None, None, "4"),
    ("yuyv", (8, 8), None, None, 130, "4"), ("rgbx", (8, 8), None, None, 258, "4"),
    ("nv12", (8, 8), (8, 9), None, None, "even"), ("nv12", (8, 8), None, (0, 65), None, "even"), ("nv12", (8, 8), None, None, 97, "even"),
]
ACCEPTED = [("rgb", (7, 9), 29, None, 301), ("bgr", (7, 9), 31, None, None), ("i420", (8, 8), (9, 5, 7), (0, 73, 101), 151),
            ("nv12", (8, 8), (9, 10), (0, 74), 200), ("yuyv", (7, 8), 20, None, 144), ("rgbx", (7, 9), 40, None, 280)]


def c_layout(code, ptrs, pitch, offsets, stride):
    from lanedetection_end2end_amd.pipeline import _CLayout
    pad3 = lambda v: tuple(v) + (0,) * (3 - len(tuple(v)))
    pitch = (pitch,) if isinstance(pitch, int) else (pitch or ())
    return _CLayout(code, ptrs, (ctypes.c_long * 3)(*pad3(pitch)), (ctypes.c_long * 3)(*pad3(offsets or ())), stride or 0)


def test_refusals_python_and_c():
    from lanedetection_end2end_amd.pipeline import FrameLayout, InputPipeline, frames_shape
    L = lib()
    jfif = (ctypes.c_int * 6)(*F.PRESETS["jfif"])
    for fmt, hw, pitch, offsets, stride, word in REFUSED:
        with pytest.raises(ValueError) as e:
            FrameLayout(fmt, hw, pitch, offsets, stride)
        assert word in str(e.value), (fmt, hw, pitch, offsets, stride, str(e.value))
        p = ctypes.c_void_p(L.lf_pipeline_plan_create(hw[0], hw[1], 0, hw[0], 4, 8))
        try:
            before = L.lf_pipeline_frame_bytes(p)
            assert before == hw[0] * hw[1] * 3
            rc = L.lf_pipeline_plan_set_layout(p, ctypes.byref(c_layout(S.FORMATS[fmt], 0, pitch, offsets, stride)), jfif)
            assert rc != 0 and b"lf_pipeline_plan_set_layout" in L.lf_last_error(), (fmt, hw, pitch, offsets, stride)
            assert L.lf_pipeline_frame_bytes(p) == before and L.lf_pipeline_surface_span(p, -1) == before, "a refused call changed the plan"
        finally:
            L.lf_pipeline_plan_destroy(p)
    with pytest.raises(ValueError, match="pixel_format"):
        FrameLayout("rgba", (8, 8))
    with pytest.raises(ValueError, match="pixel_format"):
        FrameLayout("p010", (8, 8))
    with pytest.raises(ValueError, match="pitch"):
        FrameLayout("rgb", (8, 8), pitch=(24, 24))            # more pitches than planes
    with pytest.raises(ValueError, match="pitch"):
        FrameLayout("rgb", (8, 8), pitch=24.0)
    p = ctypes.c_void_p(L.lf_pipeline_plan_create(8, 8, 0, 8, 4, 8))
    try:
        ok = c_layout(2, 0, (16, 16), None, None)
        assert L.lf_pipeline_plan_set_layout(None, ctypes.byref(ok), jfif) != 0
        assert L.lf_pipeline_plan_set_layout(p, None, jfif) != 0 and b"null" in L.lf_last_error()
        for code in (-1, 7, 77):
            assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(c_layout(code, 0, None, None, None)), jfif) != 0
            assert b"unknown format" in L.lf_last_error()
        big = (ctypes.c_int * 6)(1 << 24, 0, 1, 1, 1, 1)
        assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(ok), big) != 0 and b"int32" in L.lf_last_error()
        assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(c_layout(4, 0, None, None, None)), big) != 0
        assert L.lf_pipeline_frame_bytes(p) == 8 * 8 * 3 and L.lf_pipeline_surface_span(p, 1) == 0
        # accepted: the numbers; set_format keeps refusing the new codes, and resets a layout plan to a tight one
        assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(ok), jfif) == 0, L.lf_last_error()
        assert L.lf_pipeline_frame_bytes(p) == 8 * 16 + 4 * 16
        assert [L.lf_pipeline_surface_span(p, i) for i in (0, 1, 2, -1)] == [7 * 16 + 8, 3 * 16 + 8, 0, 8 * 16 + 3 * 16 + 8]
        for code in (4, 5, 6):
            assert L.lf_pipeline_plan_set_format(p, code, jfif) != 0 and b"unknown format" in L.lf_last_error()
        assert L.lf_pipeline_frame_bytes(p) == 8 * 16 + 4 * 16
        assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(c_layout(6, 1, None, None, None)), None) == 0      # pointer mode, NULL coef
        assert L.lf_pipeline_frame_bytes(p) == 8 * 8 * 4
        assert L.lf_pipeline_plan_set_format(p, 2, jfif) == 0
        assert L.lf_pipeline_frame_bytes(p) == 8 * 8 * 3 // 2 and L.lf_pipeline_surface_span(p, -1) == 96
        assert L.lf_pipeline_surface_span(None, 0) == 0
    finally:
        L.lf_pipeline_plan_destroy(p)
    # plane pointers: offsets and stride are not read and not looked at, whatever they hold
    for fmt, hw, pitch, offsets, stride in (("nv12", (8, 8), (9 + 1, 10), (7, -65), 97), ("yuyv", (8, 8), 20, (3,), 130), ("i420", (8, 8), (9, 5, 7), (1, 1, 1), -4)):
        lay = FrameLayout(fmt, hw, pitch, offsets, stride, plane_pointers=True)
        tight_offsets = FrameLayout(fmt, hw, pitch, plane_pointers=True)
        assert (lay.plane_offsets, lay.frame_stride, lay.span) == (tight_offsets.plane_offsets, tight_offsets.frame_stride, tight_offsets.span)
        p = ctypes.c_void_p(L.lf_pipeline_plan_create(hw[0], hw[1], 0, hw[0], 4, 8))
        try:
            assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(c_layout(S.FORMATS[fmt], 1, pitch, offsets, stride)), jfif) == 0, L.lf_last_error()
            assert tuple(L.lf_pipeline_surface_span(p, i) for i in range(lay.planes)) == lay.span
            assert L.lf_pipeline_frame_bytes(p) == lay.frame_stride
        finally:
            L.lf_pipeline_plan_destroy(p)
    for fmt, hw, pitch, offsets, stride in ACCEPTED:
        lay = FrameLayout(fmt, hw, pitch, offsets, stride)
        p = ctypes.c_void_p(L.lf_pipeline_plan_create(hw[0], hw[1], 0, hw[0], 4, 8))
        try:
            assert L.lf_pipeline_plan_set_layout(p, ctypes.byref(c_layout(S.FORMATS[fmt], 0, pitch, offsets, stride)), jfif) == 0, L.lf_last_error()
            assert tuple(L.lf_pipeline_surface_span(p, i) for i in range(lay.planes)) == lay.span
            assert L.lf_pipeline_surface_span(p, -1) == lay.frame_span and L.lf_pipeline_frame_bytes(p) == lay.frame_stride
            assert stride is None or lay.frame_stride == stride
        finally:
            L.lf_pipeline_plan_destroy(p)
    # the four names keep their errors; a layout with a pixel_format is refused; frames_shape is None for a layout
    with pytest.raises(ValueError, match="pixel_format"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format="i420")
    with pytest.raises(ValueError, match="pixel_format"):
        frames_shape("rgbx", 1, (8, 6))
    lay = FrameLayout("nv12", (20, 32), pitch=(64, 64))
    with pytest.raises(ValueError, match="pixel_format"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, pixel_format="nv12", layout=lay)
    with pytest.raises(ValueError, match="frame_hw"):
        InputPipeline(8, "bp", frame_hw=(20, 34), crop=16, layout=lay)
    with pytest.raises(ValueError, match="FrameLayout"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, layout="nv12")
    with pytest.raises(ValueError, match="int32"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, layout=lay, yuv=(1 << 24, 0, 1, 1, 1, 1))
    pipe = InputPipeline(8, "bp", frame_hw=(20, 32), crop=16, layout=lay, yuv="bt709")
    assert pipe.frames_shape is None and pipe.pixel_format == "nv12" and L.lf_pipeline_frame_bytes(pipe.handle) == 30 * 64
    with pytest.raises(ValueError, match="plane_pointers"):
        pipe.bind([])
    with pytest.raises(ValueError, match="plane_pointers"):
        InputPipeline(8, "bp", frame_hw=(20, 32), crop=16).bind([])


def test_symbols_in_header_library_table_and_integration():
    from lanedetection_end2end_amd import _lib
    header = open(os.path.join(ROOT, "include", "lanefit.h")).read()
    stub = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    top = header[:header.index("*/", header.index("#define LF_ABI_VERSION"))]
    m = re.search(r"additions since 5 \(surfaces\): ([^*]*)", top)
    assert m, "no 'additions since 5 (surfaces)' line"
    block = header[header.index("additions since 5 -- surfaces"):]
    sig = _lib._declare(lib())
    for name, nparams in SYMBOLS.items():
        assert name in m.group(1), name
        decl = re.search(r"^(int|size_t)\s+%s\(([^;]*)\);" % name, block, re.M)
        assert decl, name
        assert len(decl.group(2).split(",")) == nparams == len(sig[name][1]), name
        assert hasattr(lib(), name) and name in _lib.exported_symbols(), name
        assert name in stub, name
    assert "enum { LF_FRAME_I420 = 4, LF_FRAME_RGBX = 5, LF_FRAME_BGRX = 6 };" in block
    assert "enum { LF_FRAME_RGB = 0, LF_FRAME_BGR = 1, LF_FRAME_NV12 = 2, LF_FRAME_YUYV = 3 };" in header
    assert "typedef struct lf_frame_layout" in block and "YV12" in block and "lf_frame_layout" in stub
    assert re.search(r"#define LF_ABI_VERSION 5\b", header) and lib().lf_abi_version() == 5
    # the ctypes mirror of the struct has the header's fields, in order
    from lanedetection_end2end_amd.pipeline import _CLayout
    fields = re.findall(r"^\s+(?:int|long)\s+(\w+)", block[block.index("typedef struct lf_frame_layout"):block.index("} lf_frame_layout;")], re.M)
    assert fields == [f[0] for f in _CLayout._fields_] == ["format", "plane_pointers", "pitch", "plane_offset", "frame_stride"]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import isa_meta
    return isa_meta.compile_kernels(["lf_frame_stem.hip", "lf_pipeline.hip"], tmp_path_factory.mktemp("isa_surfaces"))


def test_surface_kernels_do_not_spill(kernels):
    resize = [k for k in kernels if "resize_surface_kernel" in k["mangled"]]
    stem = [k for k in kernels if "frame_surface_stem_kernel" in k["mangled"]]
    # <KSX, KSY, FMT> and <KSX, KSY, T, FMT>: the 7 / 7 and the generic taps, fp32 and bf16 storage, all seven formats
    for taps in ("Li7ELi7E", "Li0ELi0E"):
        for fmt in range(7):
            assert sum(("resize_surface_kernelI%sLi%dEE" % (taps, fmt)) in k["mangled"] for k in resize) == 1, (taps, fmt)
            for t in ("f", "DF16b"):
                assert sum(("frame_surface_stem_kernelI%s%sLi%dEE" % (taps, t, fmt)) in k["mangled"] for k in stem) == 1, (taps, t, fmt)
    assert len(resize) == 14 and len(stem) == 28
    for k in resize + stem:
        print("%-64s vgpr %3d agpr %3d lds %5d" % (k["mangled"][:64], k["vgpr"], k["agpr"], k["lds"]))
        assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["loop_scratch"] == 0, k
        assert k["vgpr"] + k["agpr"] <= 128, "two workgroups of 256 threads per SIMD set"
        assert k["lds"] == 0, "LDS is dynamic: the plan's bytes, the RGB layout for every format"


def test_host_program_staging_stays_inside_exact_buffers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = os.path.join(ROOT, "tests", "surface_stage_host.cpp")
    inc = os.path.join(ROOT, "lanedetection_end2end_amd", "csrc")
    variants = [("plain", ["-O2"])]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    static = ["-static-libasan", "-static-libubsan"]      # the runtime inside the program: it need not come first among shared libraries
    if subprocess.run([cxx] + san + static + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
        san += static
    if subprocess.run([cxx] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
        variants.append(("sanitized", san))
    else:
        print("the host compiler links no sanitizer runtime: the program's own asserts are the check")
    for name, flags in variants:
        exe = str(tmp_path / ("surface_stage_" + name))
        subprocess.run([cxx, "-std=c++17", "-Wall"] + flags + ["-I", inc, src, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True)      # the environment as it is
        print(name, r.stdout.strip(), r.stderr.strip()[-2000:])
        if name == "sanitized" and r.returncode != 0 and "does not come first in initial library list" in r.stderr:
            # the sanitizer's runtime refuses to start beside a library the environment loads first: nothing of the program ran.
            # The plain variant's asserts are the check then.
            print("the sanitized variant could not start in this environment; the plain variant ran")
            continue
        assert r.returncode == 0 and "pixels equal the definition" in r.stdout, (name, r.returncode)
