"""Float64 reference of the sub-pose interpolation WITH the times as tensors: V_p = matrix_exp(-t_p xi^) V, xi^ =
[[ang]x lin; 0 0], differentiated by autograd.  (oracle/gs_oracle.py::subpose_viewmats casts its times to float, so it
cannot give d loss / d time.)  Test infrastructure only."""
import torch


def xi_hat(lin: torch.Tensor, ang: torch.Tensor) -> torch.Tensor:
    z = torch.zeros((), dtype=torch.float64)
    lin, ang = lin.double(), ang.double()
    rows = [torch.stack([z, -ang[2], ang[1], lin[0]]), torch.stack([ang[2], z, -ang[0], lin[1]]),
            torch.stack([-ang[1], ang[0], z, lin[2]]), torch.zeros(4, dtype=torch.float64)]
    return torch.stack(rows)


def subpose_viewmats(viewmat: torch.Tensor, lin: torch.Tensor, ang: torch.Tensor, times: torch.Tensor) -> torch.Tensor:
    """[P,4,4] float64, differentiable in all four inputs (times [P] float64 tensor)"""
    X = xi_hat(lin, ang)
    V = viewmat.double()
    return torch.stack([torch.linalg.matrix_exp(-t * X) @ V for t in times.double().reshape(-1)])


def gradients(viewmat, lin, ang, times, v_out):
    """d <v_out, V_p> / d (viewmat, lin, ang, times) in float64; v_out [P,4,4] (row 3 ignored)"""
    V, l, a, t = (x.detach().double().clone().requires_grad_(True) for x in (viewmat, lin, ang, times))
    go = v_out.detach().double().clone()
    go[:, 3, :] = 0
    (subpose_viewmats(V, l, a, t) * go).sum().backward()
    return V.grad, l.grad, a.grad, t.grad


def rel_max(a, b) -> float:
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))
