"""fp64 restatement of the stem's data gradient (``lf_stem_bwd_data``): the gradient of
``cat[conv2d(x, w, stride=2, padding=1), max_pool2d(x, 2)]`` with respect to ``x``, written out as the gather the kernel
performs, not by autograd.

    gimg[n][ci][y][x] = sum_{co < Cc} sum_{ky,kx} [ (y+1-ky), (x+1-kx) even, oy = (y+1-ky)/2 in [0,Ho), ox = (x+1-kx)/2 in [0,Wo) ]
                                                   w[co][ci][ky][kx] * gcat[n][oy][ox][co]
                      + ( (y&1, x&1) is the arg-max of window (y>>1, x>>1) of channel ci ? gcat[n][y>>1][x>>1][Cc+ci] : 0 )

with the arg-max the first maximum in window scan order (strict >, ATen's max_pool2d rule)."""
import numpy as np


def input_grad_ref(gcat, img, w):
    """gcat (N, Ho, Wo, 16) NHWC, img (N, Cin, H, W), w (16 - Cin, Cin, 3, 3) -> (R, S), both (N, Cin, H, W) float64:
    the gradient and the magnitude sum  S = sum |w| |g| + |g_pool|  of the terms that make up each element."""
    g = np.asarray(gcat, dtype=np.float64)
    x = np.asarray(img, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, Cin, H, W = x.shape
    Cc = 16 - Cin
    Ho, Wo = H // 2, W // 2
    assert g.shape == (N, Ho, Wo, 16) and w.shape == (Cc, Cin, 3, 3) and H % 2 == 0 and W % 2 == 0
    R = np.zeros((N, Cin, H, W))
    S = np.zeros((N, Cin, H, W))
    gc = g[..., :Cc]                                        # (N, Ho, Wo, Cc)
    for ky in range(3):
        for kx in range(3):
            # image pixel (y, x) = (2 oy + ky - 1, 2 ox + kx - 1) lies in the patch of output pixel (oy, ox) at tap (ky, kx)
            oy = np.arange(Ho)
            ox = np.arange(Wo)
            y, xx = 2 * oy + ky - 1, 2 * ox + kx - 1
            oy, y = oy[(y >= 0) & (y < H)], y[(y >= 0) & (y < H)]
            ox, xx = ox[(xx >= 0) & (xx < W)], xx[(xx >= 0) & (xx < W)]
            sub = gc[:, oy][:, :, ox]                       # (N, ny, nx, Cc)
            wt = w[:, :, ky, kx]                            # (Cc, Cin)
            R[:, :, y[:, None], xx[None, :]] += np.einsum("nyxo,oc->ncyx", sub, wt)
            S[:, :, y[:, None], xx[None, :]] += np.einsum("nyxo,oc->ncyx", np.abs(sub), np.abs(wt))
    win = x.reshape(N, Cin, Ho, 2, Wo, 2).transpose(0, 1, 2, 4, 3, 5).reshape(N, Cin, Ho, Wo, 4)    # scan order (0,0) (0,1) (1,0) (1,1)
    arg = np.zeros((N, Cin, Ho, Wo), dtype=np.int64)
    m = win[..., 0].copy()
    for j in (1, 2, 3):
        better = win[..., j] > m                            # strict: the first maximum wins
        arg[better] = j
        m[better] = win[..., j][better]
    gp = g[..., Cc:].transpose(0, 3, 1, 2)                  # (N, Cin, Ho, Wo)
    for j in range(4):
        a, b = j >> 1, j & 1
        R[:, :, a::2, b::2] += np.where(arg == j, gp, 0.0)
        S[:, :, a::2, b::2] += np.where(arg == j, np.abs(gp), 0.0)
    return R, S
