"""fp64 references of the bandwidth-bound backbone kernels (BatchNorm finalise / apply / backward, max-pool branch, stem, head,
1x1 convolution), written from the contracts in csrc/lf_eltwise.h / csrc/lf_debug.h and from BEV/Networks/ERFNet.py -- NOT from the
kernels: the statistics are merged with Chan's pairwise update of (n, mean, M2) (the kernels add sums of squares about the origin),
the pool arg-max is an explicit scan, the convolutions are explicit sums over taps (no F.conv*: tests/test_eltwise_ref_cpu.py
compares every function here with torch's own operator, so a misread contract cannot sit on both sides of a GPU comparison).

Everything is torch fp64 on the device of its operands (the statistics merge: the CPU); tensors are NHWC unless a name says nchw.
Functions that a tolerance needs return, or can be called to return, the sum of absolute values of the terms of every output (`S`):
call them with absolute-valued operands.
"""
import torch

EPS = 1e-3          # nn.BatchNorm2d(eps=1e-3) everywhere in ERFNet.py
MOMENTUM = 0.1


def f64(t):
    return None if t is None else t.detach().to(torch.float64)


# ---- BatchNorm statistics -------------------------------------------------------------------------------------------------------

def row_pixels(nrows, tile_pix, seg_rows, seg_pix):
    """n_r of the centred rows of a tap-GEMM launch: row r covers pixels (r % seg_rows) * tile_pix .. of seg_pix."""
    r = torch.arange(nrows, dtype=torch.float64) % seg_rows
    return torch.clamp(seg_pix - r * tile_pix, max=float(tile_pix))


def row_triples(kind0, kind1, n, centred):
    """(n_r, mean_r, M2_r), each [C, R], of partial rows: kind0 = sum v; kind1 = M2 (centred) or sum v^2 (raw: M2 = sum v^2 - (sum v)^2 / n)."""
    kind0, kind1 = f64(kind0), f64(kind1)
    n = f64(n).expand_as(kind0)
    m2 = kind1 if centred else kind1 - kind0 * kind0 / n
    return n.clone(), kind0 / n, m2.clone()


def chan_merge(n, mean, m2):
    """Chan et al.'s pairwise merge over the last axis of [C, R] triples -> (n, mean, M2), each [C]."""
    while n.shape[1] > 1:
        if n.shape[1] & 1:
            z = torch.zeros(n.shape[0], 1, dtype=torch.float64)
            n, mean, m2 = torch.cat([n, z], 1), torch.cat([mean, z], 1), torch.cat([m2, z], 1)
        na, nb, ma, mb = n[:, 0::2], n[:, 1::2], mean[:, 0::2], mean[:, 1::2]
        nt = na + nb
        w = torch.where(nt > 0, nb / nt.clamp(min=1.0), torch.zeros_like(nt))
        d = mb - ma
        n, mean, m2 = nt, ma + d * w, m2[:, 0::2] + m2[:, 1::2] + d * d * na * w
    return n[:, 0], mean[:, 0], m2[:, 0]


def batch_stats(sources, C):
    """sources: dicts (kind0 [Ci, R], kind1 [Ci, R], n [R], centred, ch_off).  -> (n, mean, biased var) [C]; a channel that no source
    covers has n = 0, mean 0, var 0.  The variance is clamped at 0 (rounded raw rows of a constant channel)."""
    n, mean, var = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    for s in sources:
        a, b, c = chan_merge(*row_triples(s["kind0"], s["kind1"], s["n"], s["centred"]))
        sl = slice(s["ch_off"], s["ch_off"] + a.numel())
        assert bool((n[sl] == 0).all()), "two sources cover one channel"
        n[sl], mean[sl], var[sl] = a, b, torch.clamp(c / a, min=0.0)
    return n, mean, var


def bn_finalize_fwd(mean, var, count, gamma, beta, rmean, rvar, training, momentum=MOMENTUM, eps=EPS):
    """mean / biased var [C] of the batch (ignored in eval mode).  -> dict of scale, shift, asc (rstd), ash (-mean * rstd), rmean, rvar,
    and the |terms| sums S_* of each for the tolerances."""
    gamma, beta, rmean, rvar = f64(gamma), f64(beta), f64(rmean), f64(rvar)
    o = {}
    if training:
        unb = var * count / (count - 1.0) if count > 1 else var
        o["rmean"], o["S_rmean"] = (1 - momentum) * rmean + momentum * mean, (1 - momentum) * rmean.abs() + momentum * mean.abs()
        o["rvar"], o["S_rvar"] = (1 - momentum) * rvar + momentum * unb, (1 - momentum) * rvar.abs() + momentum * unb.abs()
    else:
        mean, var = rmean, rvar
        o["rmean"], o["rvar"] = rmean, rvar
    rstd = 1.0 / torch.sqrt(var + eps)
    o["asc"], o["S_asc"] = rstd, rstd
    o["ash"], o["S_ash"] = -mean * rstd, (mean * rstd).abs()
    o["scale"], o["S_scale"] = gamma * rstd, (gamma * rstd).abs()
    o["shift"], o["S_shift"] = beta - mean * gamma * rstd, beta.abs() + (mean * gamma * rstd).abs()
    return o


def image_of_pixel(npix, pix_per_image, device):
    return torch.arange(npix, device=device) // pix_per_image


def bn_act(x, sc, sh, dm, res, pix_per_image):
    """x, res [npix, C]; dm [images, C] or None.  relu((x * sc + sh) * dm + res)."""
    v = f64(x) * f64(sc) + f64(sh)
    if dm is not None:
        v = v * f64(dm)[image_of_pixel(x.shape[0], pix_per_image, x.device)]
    if res is not None:
        v = v + f64(res)
    return torch.relu(v)


def masked_grad(g, y, dm, pix_per_image):
    """gm = g * [y > 0] * dm, and gz = g * [y > 0] (the residual branch's gradient)."""
    gz = f64(g) if y is None else f64(g) * (f64(y) > 0)
    gm = gz if dm is None else gz * f64(dm)[image_of_pixel(g.shape[0], pix_per_image, g.device)]
    return gm, gz


def bn_bwd_sums(g, y, t, dm, pix_per_image):
    """column sums (sum gm, sum gm * t) [C] -- what the reduce kernel's partial rows add up to."""
    gm, _ = masked_grad(g, y, dm, pix_per_image)
    return gm.sum(0), (gm * f64(t)).sum(0)


def bn_bwd_finalize(s1, s2, asc, ash, count, training):
    """s1, s2 = the column sums (sum gm, sum gm * t).  -> c1, c2, ggamma = sum gm * xhat, gbeta; c1 = c2 = 0 in eval mode."""
    asc, ash = f64(asc), f64(ash)
    ggamma, gbeta = asc * s2 + ash * s1, s1
    k = 1.0 / count if training else 0.0
    return {"c1": gbeta * k, "c2": ggamma * k, "ggamma": ggamma, "gbeta": gbeta}


def bn_bwd_apply(g, y, t, asc, ash, gamma, c1, c2, dm, pix_per_image):
    """-> g_t = gamma * rstd * (gm - c1 - xhat * c2), g_z, and S (the |terms| sum of g_t)."""
    gm, gz = masked_grad(g, y, dm, pix_per_image)
    asc, ash, gamma, c1, c2, t = f64(asc), f64(ash), f64(gamma), f64(c1), f64(c2), f64(t)
    gt = gamma * asc * (gm - c1 - (t * asc + ash) * c2)
    S = (gamma * asc).abs() * (gm.abs() + c1.abs() + ((t * asc).abs() + ash.abs()) * c2.abs())
    return gt, gz, S


# ---- max-pool branch ------------------------------------------------------------------------------------------------------------

def pool_windows(x):
    """x [N, H, W, C] -> [N, H/2, W/2, C, 4], the window in the scan order (0,0), (0,1), (1,0), (1,1)."""
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]], -1)


def pool_argmax(x):
    """explicit scan: the first maximum wins (a later element replaces it only when strictly greater) -> (max, index in scan order)."""
    w = pool_windows(x)
    m, arg = w[..., 0].clone(), torch.zeros(w.shape[:-1], dtype=torch.long, device=x.device)
    for k in (1, 2, 3):
        better = w[..., k] > m
        m = torch.where(better, w[..., k], m)
        arg = torch.where(better, torch.full_like(arg, k), arg)
    return m, arg


def pool_bwd(x, gpool):
    """gx [N, H, W, C] in the dtype of gpool: gpool at the window's arg-max, +0 elsewhere."""
    _, arg = pool_argmax(x)
    gx = torch.zeros(x.shape, dtype=gpool.dtype, device=x.device)
    for k, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        gx[:, a::2, b::2] = torch.where(arg == k, gpool, torch.zeros_like(gpool))
    return gx


def pool_affine(x, sc, sh):
    return torch.relu(pool_argmax(f64(x))[0] * f64(sc) + f64(sh))


# ---- stem: DownsamplerBlock(Cin, 16) on the NCHW image ------------------------------------------------------------------------------

def stem_conv(img_nchw, w, b):
    """Conv2d(Cin, Cout, 3, stride 2, padding 1) as an explicit sum over taps -> NHWC [N, H/2, W/2, Cout]."""
    x, w, b = f64(img_nchw), f64(w), f64(b)
    N, Cin, H, W = x.shape
    xp = torch.zeros(N, Cin, H + 2, W + 2, dtype=torch.float64, device=x.device)
    xp[:, :, 1:-1, 1:-1] = x
    out = b.view(1, 1, 1, -1).expand(N, H // 2, W // 2, w.shape[0]).clone()
    for kh in range(3):
        for kw in range(3):
            patch = xp[:, :, kh:kh + H:2, kw:kw + W:2]                    # image rows 2 oy + kh - 1, columns 2 ox + kw - 1
            out += torch.einsum("ncyx,oc->nyxo", patch, w[:, :, kh, kw])
    return out


def stem(img_nchw, w, b):
    """cat [N, H/2, W/2, 16] = [conv | maxpool2x2 of the image's channels]."""
    return torch.cat([stem_conv(img_nchw, w, b), pool_argmax(f64(img_nchw).permute(0, 2, 3, 1))[0]], -1)


def stem_abs(img_nchw, w, b):
    """sum |w x| + |b| for the convolution channels, |v| for the pooled ones."""
    return stem(f64(img_nchw).abs(), f64(w).abs(), f64(b).abs())


# ---- head: ConvTranspose2d(16, K, 2, stride 2) ----------------------------------------------------------------------------------------

def head_fwd(x, w, b):
    """x [N, h, w, 16], w [16, K, 2, 2], b [K] -> NCHW [N, K, 2h, 2w]: stride = kernel, every output pixel has ONE input pixel."""
    x, w, b = f64(x), f64(w), f64(b)
    N, h, wd, _ = x.shape
    out = torch.empty(N, w.shape[1], 2 * h, 2 * wd, dtype=torch.float64, device=x.device)
    for a in range(2):
        for c in range(2):
            out[:, :, a::2, c::2] = torch.einsum("nijc,ck->nkij", x, w[:, :, a, c]) + b.view(1, -1, 1, 1)
    return out


def head_bwd_data(gout_nchw, w):
    g, w = f64(gout_nchw), f64(w)
    gx = 0
    for a in range(2):
        for c in range(2):
            gx = gx + torch.einsum("nkij,ck->nijc", g[:, :, a::2, c::2], w[:, :, a, c])
    return gx


# ---- encoder.output_conv: Conv2d(C, K, 1) -----------------------------------------------------------------------------------------

def pointwise_fwd(x, w, b):
    """x [N, h, w, C], w [K, C], b [K] or None -> NCHW [N, K, h, w]."""
    y = torch.einsum("nijc,kc->nkij", f64(x), f64(w))
    return y if b is None else y + f64(b).view(1, -1, 1, 1)


def pointwise_bwd(x, gy_nchw, w):
    """-> gx [N, h, w, C], gw [K, C], gb [K]."""
    x, g, w = f64(x), f64(gy_nchw), f64(w)
    return torch.einsum("nkij,kc->nijc", g, w), torch.einsum("nkij,nijc->kc", g, x), g.sum((0, 2, 3))
