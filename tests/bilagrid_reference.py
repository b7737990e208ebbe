"""TEST INFRASTRUCTURE ONLY: the float64 reference of the bilateral-grid colour correction, as upstream evaluates it — one
5-D torch.nn.functional.grid_sample(mode="bilinear", padding_mode="border", align_corners=True) and autograd —, and the
total variation with tensor slicing.  Shares no code with the product (3dgs-deblur_amd/bilagrid.py,
csrc/bilagrid_math.h)."""
import torch
import torch.nn.functional as F


def slice_ref(grids, rgb, grid_idx, dtype=torch.float64):
    """grids [G,12,L,GH,GW], rgb [B,H,W,3], grid_idx: B ints -> corrected [B,H,W,3] in `dtype` (differentiable)"""
    grids, rgb = grids.to(dtype), rgb.to(dtype)
    B, H, W, _ = rgb.shape
    u = (torch.arange(W, dtype=dtype) + 0.5) / W
    v = (torch.arange(H, dtype=dtype) + 0.5) / H
    guide = 0.299 * rgb[..., 0] + 0.587 * rgb[..., 1] + 0.114 * rgb[..., 2]
    coords = torch.stack([u.view(1, 1, W).expand(B, H, W), v.view(1, H, 1).expand(B, H, W), guide], dim=-1)
    coords = coords * 2.0 - 1.0                                      # grid_sample's [-1, 1]; order (x -> GW, y -> GH, z -> L)
    per_image = grids[torch.as_tensor(list(grid_idx), dtype=torch.long)]
    affine = F.grid_sample(per_image, coords[:, None], mode="bilinear", padding_mode="border", align_corners=True)
    affine = affine[:, :, 0].permute(0, 2, 3, 1).reshape(B, H, W, 3, 4)
    return torch.einsum("bhwij,bhwj->bhwi", affine[..., :3], rgb) + affine[..., 3]


def slice_ref_grads(grids, rgb, grid_idx, v_out, dtype=torch.float64):
    """-> (out, v_rgb, v_grids) of slice_ref under the cotangent v_out"""
    g = grids.detach().to(dtype).requires_grad_(True)
    r = rgb.detach().to(dtype).requires_grad_(True)
    out = slice_ref(g, r, grid_idx, dtype)
    v_rgb, v_grids = torch.autograd.grad(out, (r, g), v_out.to(dtype))
    return out.detach(), v_rgb, v_grids


def tv_ref(grids, dtype=torch.float64):
    g = grids.to(dtype)
    mx = ((g[:, :, :, :, 1:] - g[:, :, :, :, :-1]) ** 2).mean()
    my = ((g[:, :, :, 1:, :] - g[:, :, :, :-1, :]) ** 2).mean()
    mz = ((g[:, :, 1:, :, :] - g[:, :, :-1, :, :]) ** 2).mean()
    return 2.0 * (mx + my + mz)


def tv_ref_grads(grids, weight, dtype=torch.float64):
    g = grids.detach().to(dtype).requires_grad_(True)
    t = weight * tv_ref(g, dtype)
    (v,) = torch.autograd.grad(t, g)
    return t.detach(), v


def fragile_pixels(rgb, L, eps=1e-4):
    """[B,H,W] bool: luma * (L - 1) within eps of an integer — there the guide gradient jumps from one pair of L-slices
    to the next (and, at 0 and L - 1, between clamped and not), so v_rgb of the two sides differs by a finite amount"""
    p = (0.299 * rgb[..., 0].double() + 0.587 * rgb[..., 1].double() + 0.114 * rgb[..., 2].double()) * (L - 1)
    return (p - p.round()).abs() <= eps


def random_case(B, H, W, G, shape, seed, wide=True):
    """seeded inputs: grids around the identity with every channel perturbed, colours uniform in [-0.15, 1.15] (wide: some
    lumas below 0 and above 1) or [0, 1], a cotangent of unit scale"""
    GW, GH, L = shape
    g = torch.Generator().manual_seed(seed)
    eye = torch.tensor([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]).view(1, 12, 1, 1, 1)
    grids = (eye + 0.3 * torch.randn(G, 12, L, GH, GW, generator=g)).float()
    rgb = torch.rand(B, H, W, 3, generator=g)
    if wide:
        rgb = rgb * 1.3 - 0.15
        rgb[:, 0, 0, :] = torch.tensor([1.12, 1.05, 1.2])          # at least one guide above 1 ...
        rgb[:, -1, -1, :] = torch.tensor([-0.08, -0.02, -0.11])    # ... and one below 0, whatever the size
    v_out = torch.randn(B, H, W, 3, generator=g).float()
    return grids, rgb.float().contiguous(), v_out
