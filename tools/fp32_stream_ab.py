#!/usr/bin/env python
"""tapstream_kernel against tapgemm_kernel on the same launches (fp32 3-tap C -> C convolutions at batch 32, the shapes of the BEV
headline): every variant the stream kernel is compiled for, forward and transposed weights, HIP-event timed in alternated rounds
(lf_debug_set_fp32_stream 0 / 2), results compared bit for bit.  Each call also runs the weight pack kernel (a few us, in both).

    python tools/fp32_stream_ab.py [--iters 200] [--rounds 3] [--batch 32]
"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lanedetection_end2end_amd import _lib  # noqa: E402


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def timeit(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    lib = _lib.load()
    st = _lib.stream()
    N = a.batch
    try:
        for C, H, W, axis, d in ((64, 64, 128, 1, 1), (64, 64, 128, 0, 1), (128, 32, 64, 1, 16), (128, 32, 64, 0, 4)):
            torch.manual_seed(0)
            x = torch.randn(N, H, W, C, device="cuda")
            mask = torch.randn(N, H, W, C, device="cuda")
            w = torch.randn(C, C, 3, device="cuda") * (2.0 / (3 * C)) ** 0.5
            b = torch.randn(C, device="cuda")
            sc, sh = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda") * 0.5
            scratch = torch.empty(lib.lf_conv1d_scratch_floats(N, H, W, C), device="cuda")
            nrows = (N * H * W + 255) // 256
            stats = torch.empty(2 * C * nrows, device="cuda")
            y = torch.empty_like(x)
            add, aux = torch.randn(N, H, W, C, device="cuda"), torch.randn(N, H, W, C, device="cuda")
            epi = lambda tr, e, bias, m: (lambda: lib.lf_debug_conv1d_epi(P(x), P(w), P(bias), P(y), tr, e, P(m), P(add) if e & 4 else None, P(aux) if e & 48 else None,
                                                                         P(sc) if e & 16 else None, P(sh) if e & 16 else None,
                                                                         P(stats) if e & 40 else None, N, H, W, C, axis, d, P(scratch), st))
            launches = [("fwd + relu", epi(0, 1, b, None)), ("fwd + BN sums", epi(0, 8, b, None)), ("dgrad * mask", epi(1, 2, None, mask)),
                        ("dgrad + relu", epi(1, 1, None, None)), ("dgrad * BN mask + sums", epi(1, 48, None, None)),
                        ("(dgrad + add) * mask + sums", epi(1, 38, None, mask)),
                        ("bn-relu prologue + relu", lambda: lib.lf_debug_conv1d_fwd_pro(P(x), P(w), P(b), P(sc), P(sh), P(y), N, H, W, C, axis, d, P(scratch), st))]
            for name, fn in launches:
                t = {0: [], 2: []}
                outs = {}
                for _ in range(a.rounds):
                    for mode in (0, 2):
                        lib.lf_debug_set_fp32_stream(mode, 0)
                        t[mode].append(timeit(fn, a.iters))
                        outs[mode] = (y.clone(), stats.clone())
                same = torch.equal(outs[0][0], outs[2][0]) and ("sums" not in name or torch.equal(outs[0][1], outs[2][1]))
                m0, m2 = sorted(t[0])[len(t[0]) // 2], sorted(t[2])[len(t[2]) // 2]
                print("C=%3d %3dx%3d axis %d dil %2d %-24s | tapgemm %6.1f us (%s) | tapstream %6.1f us (%s) | %+5.1f us | bits %s"
                      % (C, H, W, axis, d, name, m0, " ".join("%.1f" % v for v in t[0]), m2, " ".join("%.1f" % v for v in t[2]), m2 - m0,
                         "equal" if same else "DIFFER"), flush=True)
    finally:
        lib.lf_debug_set_fp32_stream(1, 0)


if __name__ == "__main__":
    main()
