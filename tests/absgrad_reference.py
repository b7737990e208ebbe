"""Float64 per-pair reference of the screen-space centre gradient: signed sum AND absgrad.

Autograd through the oracle's ``rasterize_sorted`` only yields the SIGNED per-Gaussian sum of d loss / d xy.  Absgrad
takes the absolute value of every (pixel, Gaussian) pair's contribution, per component, before any sum, so it needs the
pairs themselves.  ``absgrad_part`` recomputes one sub-pose's composite per tile from the oracle's parts
(``O.render(..., return_parts=True)``) with the oracle's own decisions (validity, clamp, the T > 1e-4 stop) and applies
the backward formulas of SURVEY.md App. A per pair:

    v_alpha_i = T_i (c_i . v_C) - (sum_{j>i} w_j (c_j . v_C) + T_final (bg . v_C)) / (1 - alpha_i)
    v_sigma_i = -o_i e^{-sigma_i} v_alpha_i                  (zero where the clamp is active, unless UP_ALPHA_CLAMP)
    d loss / d x_i = v_sigma_i (cxx dx + cxy dy),   d loss / d y_i = v_sigma_i (cxy dx + cyy dy)

Its signed sum is checked against autograd (tests/test_absgrad_host.py), which is what lets the GPU tests use its
absolute sum as the reference.
"""
import numpy as np
import torch


def absgrad_part(O, xys, conics, colors, opac, gids, bins, H, W, v_img, tile_rows=None, upstream=None, background=None):
    """One sub-pose.  v_img [H,W,3] = d loss / d image of this sub-pose's sample; -> (signed [N,2], abs [N,2]) float64:
    the sums over the pixels of d loss / d xy of every (pixel, Gaussian) pair, and of its absolute value"""
    upstream = O.DEFAULT_GRADS if upstream is None else upstream
    dt = torch.float64
    TILE = O.TILE
    N = xys.shape[0]
    sg = torch.zeros(N, 2, dtype=dt)
    ab = torch.zeros(N, 2, dtype=dt)
    tiles_x, tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ty0, ty1 = (0, tiles_y) if tile_rows is None else tile_rows
    opac = opac.reshape(-1)
    C = colors.shape[1]             # 3; any channel count works as long as colours, v_img and background agree
    bg = torch.zeros(C, dtype=dt) if background is None else background.to(dt)
    for ty in range(ty0, ty1):
        for tx in range(tiles_x):
            t = ty * tiles_x + tx
            s, e = int(bins[t, 0]), int(bins[t, 1])
            if e <= s:
                continue
            y_lo, y_hi = ty * TILE, min((ty + 1) * TILE, H)
            x_lo, x_hi = tx * TILE, min((tx + 1) * TILE, W)
            hh, ww = y_hi - y_lo, x_hi - x_lo
            ids = torch.from_numpy(gids[s:e].astype(np.int64))
            PX = (torch.arange(x_lo, x_hi, dtype=dt) + 0.5)[None, :].expand(hh, ww).reshape(-1)
            PY = (torch.arange(y_lo, y_hi, dtype=dt) + 0.5)[:, None].expand(hh, ww).reshape(-1)
            dx = xys[ids, 0][:, None] - PX[None]
            dy = xys[ids, 1][:, None] - PY[None]
            cxx, cxy, cyy = conics[ids, 0][:, None], conics[ids, 1][:, None], conics[ids, 2][:, None]
            sigma = 0.5 * (cxx * dx * dx + cyy * dy * dy) + cxy * dx * dy
            ov = opac[ids][:, None] * torch.exp(-sigma)
            alpha = torch.clamp(ov, max=O.ALPHA_MAX)
            valid = (sigma >= 0) & (alpha >= O.ALPHA_MIN)
            a = torch.where(valid, alpha, torch.zeros_like(alpha))
            Tincl = torch.cumprod(1 - a, 0)
            Texcl = torch.cat([torch.ones_like(Tincl[:1]), Tincl[:-1]], 0)
            live = Tincl > O.T_MIN
            on = valid & live
            w = a * Texcl * on.to(dt)
            Tfin = torch.clamp(torch.where(live, Tincl, torch.full_like(Tincl, 2.0)).min(dim=0).values, max=1.0)
            vC = v_img[y_lo:y_hi, x_lo:x_hi].reshape(-1, C).to(dt)        # [px,C]
            cv = colors[ids] @ vC.T                                        # [n,px]  c_i . v_C
            wc = w * cv
            behind = torch.flip(torch.cumsum(torch.flip(wc, [0]), 0), [0]) - wc + (Tfin * (vC @ bg))[None]
            v_alpha = torch.where(on, Texcl * cv - behind / (1 - a), torch.zeros_like(a))
            ovm = ov if (upstream & O.UP_ALPHA_CLAMP) else torch.where(ov <= O.ALPHA_MAX, ov, torch.zeros_like(ov))
            v_sigma = -ovm * v_alpha
            gx = v_sigma * (cxx * dx + cxy * dy)
            gy = v_sigma * (cxy * dx + cyy * dy)
            sg.index_add_(0, ids, torch.stack([gx.sum(1), gy.sum(1)], -1))
            ab.index_add_(0, ids, torch.stack([gx.abs().sum(1), gy.abs().sum(1)], -1))
    return sg, ab


def frame_absgrad(O, cfg, parts, v_samples, background=None, upstream=None):
    """A whole frame of S x R sub-poses (the parts of O.render(cfg, ..., return_parts=True)); v_samples [S,H,W,3] =
    d loss / d sample images.  -> (signed [N,2], abs [N,2]) summed over the sub-poses"""
    H, W = cfg.img_height, cfg.img_width
    _, samp, band = O.subpose_times(cfg.blur_samples, cfg.exposure_time, cfg.rs_bands, cfg.rolling_shutter_time)
    rows = O.band_tile_rows(H, cfg.rs_bands)
    up = int(cfg.upstream_grads) if upstream is None else upstream
    tot_s = tot_a = None
    for p, (pr, keys, gids, bins, r, rgb, op) in enumerate(parts):
        sg, ab = absgrad_part(O, pr.xys.detach(), pr.conics.detach(), rgb.detach(), op.detach(), gids, bins, H, W,
                              v_samples[samp[p]].detach(), tile_rows=rows[band[p]], upstream=up, background=background)
        tot_s = sg if tot_s is None else tot_s + sg
        tot_a = ab if tot_a is None else tot_a + ab
    return tot_s, tot_a
