"""The split of the lane fit's translation unit, the part that needs no GPU: every kernel sits in the device code of the one file
that owns it (the kernels live in anonymous namespaces or are templates, so a copy left behind in another file would link silently),
the moved kernels do not spill, and the error buffer of ``lf_error.hip`` is the one every other object writes."""
import glob
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LOSSES = {"area_loss_kernel", "mse_loss_kernel", "backproj_kernel", "ce_fwd_kernel", "ce_finish_kernel", "ce_bwd_kernel",
          "trapezoid_kernel"}
LANES = {"lane_decode_kernel", "lane_eval_kernel", "lane_eval_totals_kernel", "lane_decode_bev_kernel"}
OWNER = {"lf_losses.hip": LOSSES,
         "lf_lanes.hip": LANES,
         "lf_fit.hip": {"wls_moments_kernel", "wls_solve_kernel", "wls_bwd_kernel", "wls_bwd_grid_kernel", "gels_moments_kernel",
                        "gels_solve_kernel", "gels_bwd_kernel", "head_moments_kernel", "segfit_kernel", "theta_grid_kernel",
                        "theta_grid_bwd_kernel", "theta_finish_kernel"},
         "lf_criterion.hip": {"step_loss_kernel", "step_scale_kernel"},
         "lf_seg_step.hip": {"seg_label_kernel", "seg_step_kernel", "seg_finish_kernel", "seg_flag_maps_kernel", "seg_scale_kernel"}}


@pytest.fixture(scope="module")
def by_file(tmp_path_factory):
    """{file: kernels of its device code}: the five files compiled once, together."""
    import isa_meta
    tmp = tmp_path_factory.mktemp("isa_fit_split")
    merged = isa_meta.compile_kernels(list(OWNER), tmp)
    out = {}
    for n in OWNER:
        (asm,) = glob.glob(os.path.join(str(tmp), n[:-4] + "-hip-*gfx950*.s"))
        out[n] = isa_meta.kernels(asm)
    assert sum(len(v) for v in out.values()) == len(merged)
    return out


def base(name):
    """The kernel's name without template arguments (a bf16 instantiation stays mangled where c++filt does not know DF16b)."""
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", name)
    if m:
        return name[m.end():m.end() + int(m.group(1))]
    return re.sub(r"<.*", "", name)


def test_every_kernel_in_its_own_file_only(by_file):
    for n, kernels in by_file.items():
        assert {base(k["name"]) for k in kernels} == OWNER[n], (n, sorted(k["name"] for k in kernels))
    names = {n: sorted(k["name"] for k in by_file[n]) for n in ("lf_losses.hip", "lf_lanes.hip")}
    assert names["lf_losses.hip"] == sorted(
        ["area_loss_kernel<double>", "area_loss_kernel<float>", "mse_loss_kernel<double>", "mse_loss_kernel<float>", "backproj_kernel",
         "ce_fwd_kernel", "ce_finish_kernel", "ce_bwd_kernel", "trapezoid_kernel<double>", "trapezoid_kernel<float>"])
    assert names["lf_lanes.hip"] == sorted(["lane_decode_kernel", "lane_eval_kernel", "lane_eval_totals_kernel",
                                            "lane_decode_bev_kernel<double>", "lane_decode_bev_kernel<float>"])


def test_moved_kernels_do_not_spill(by_file):
    for n in ("lf_losses.hip", "lf_lanes.hip"):
        for k in by_file[n]:
            print("%-14s %-34s vgpr %3d agpr %3d lds %5d" % (n, k["name"], k["vgpr"], k["agpr"], k["lds"]))
            assert k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, (n, k)


def test_error_buffer_is_shared_across_objects():
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    table = _lib.exported_symbols()
    for name in ("lf_last_error", "lf_abi_version"):
        assert hasattr(lib, name) and name in table, name
    assert lib.lf_abi_version() == 5
    src = lambda f: open(os.path.join(ROOT, "lanedetection_end2end_amd", "csrc", f)).read()
    assert "lf_last_error" in src("lf_error.hip") and "lf_erfnet_plan_create" not in src("lf_error.hip")
    assert re.search(r"^lf_erfnet_plan\* lf_erfnet_plan_create\(", src("lf_erfnet.hip"), re.M)
    # a failing call through an entry of another object: its message is what lf_last_error (lf_error.hip) returns
    assert not lib.lf_erfnet_plan_create(1, 100, 200, 3, 2, 1)        # H % 16 != 0
    assert b"unsupported" in lib.lf_last_error()
    bad = lib.lf_step_loss_bwd(None, 1, 0, 0, None, None, None)
    assert bad != 0 and lib.lf_last_error() == b"lf_step_loss_bwd: bad arguments"
