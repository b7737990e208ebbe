"""float64 restatement of the 3DGS-MCMC math (csrc/mcmc_math.h) for the tests: Philox4x32-10 in Python integers, the
Box-Muller normals, the noise displacement and the relocation correction with exact binomials (math.comb).  Formulas
recollected from gsplat 1.x relocation.cu / strategy/ops.py.  Does not import the product."""
import math

import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
MAX_RATIO = 51


def philox4x32_10(counter, key):
    c = [int(x) & MASK for x in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & MASK, (p0 >> 32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def row_words(row, seed, step):
    """counter (row, 0, step_lo, step_hi), key (seed_lo, seed_hi)"""
    return philox4x32_10([row, 0, step & MASK, (step >> 32) & MASK], [seed & MASK, (seed >> 32) & MASK])


def normals_from_words(words):
    """words int64 [N,4] -> float64 [N,3]: u = (x + 0.5) 2^-32, Box-Muller.  u is rounded to float32 the way the header
    forms it (float(x) + 0.5f, times 2^-32) and everything after it runs in float64 — "the same fp32 inputs": near
    u = 1 the radius sqrt(-2 ln u) amplifies u's rounding without bound (u = 1 - 2^-33 gives 1.5e-5, float32's u = 1
    gives 0), which says nothing about the code under test"""
    u = ((words.float() + 0.5) * torch.tensor(2.0 ** -32, dtype=torch.float32)).double()
    r0, r1 = torch.sqrt(-2 * torch.log(u[:, 0])), torch.sqrt(-2 * torch.log(u[:, 2]))
    return torch.stack([r0 * torch.cos(2 * math.pi * u[:, 1]), r0 * torch.sin(2 * math.pi * u[:, 1]),
                        r1 * torch.cos(2 * math.pi * u[:, 3])], dim=-1)


def noise_delta(log_scales, quats, logits, z, scaler):
    """Sigma (z gate scaler) in float64 from the given (float32) inputs; quats wxyz, unnormalised"""
    ls, q, l, z = log_scales.double(), quats.double(), logits.double().reshape(-1), z.double()
    o = 1.0 / (1.0 + torch.exp(-l))
    gate = 1.0 / (1.0 + torch.exp(100.0 * (o - 0.005)))
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, zz = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - w * zz), 2 * (x * zz + w * y),
                     2 * (x * y + w * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - w * x),
                     2 * (x * zz - w * y), 2 * (y * zz + w * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    S2 = torch.diag_embed(torch.exp(ls) ** 2)
    cov = R @ S2 @ R.transpose(1, 2)
    return (cov @ (z * (gate * float(scaler))[:, None])[..., None]).squeeze(-1)


def relocation(opacities, scales, ratios):
    """o' = 1 - (1 - o)^(1/n); D = sum_{i=1..n} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1); s' = s o / D;
    n = ratios clamped to [1, 51].  float64, exact binomials."""
    o = opacities.double().reshape(-1)
    s = scales.double()
    n_all = ratios.to(torch.int64).reshape(-1).clamp(1, MAX_RATIO)
    new_o = torch.empty_like(o)
    D = torch.zeros_like(o)
    for n in sorted(set(n_all.tolist())):
        sel = n_all == n
        op = 1.0 - (1.0 - o[sel]) ** (1.0 / n)
        new_o[sel] = op
        d = torch.zeros_like(op)
        for i in range(1, n + 1):
            for k in range(i):
                d = d + math.comb(i - 1, k) * (-1.0) ** k * op ** (k + 1) / math.sqrt(k + 1)
        D[sel] = d
    return new_o, s * (o / D)[:, None]
