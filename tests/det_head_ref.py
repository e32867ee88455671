"""numpy restatement of the deterministic decoder's head (hulc/models/decoders/deterministic_decoder.py): Linear(2048, 7) + tanh, nn.HuberLoss / nn.MSELoss
(reduction "mean"), both target frames, and the head's three gradients.  Every function runs in the dtype of its arrays: float64 is the reference of the GPU
tests, float32 on the same operands measures their gates (tests/det_head_inputs.py).  Rows are whatever order the caller uses, the same for every argument."""
import numpy as np

from enc_head_ref import _euler_xyz, world_to_tcp

HUBER, MSE = 0, 1


def tcp_to_world(action, robot_obs):
    """tcp-frame action (.., 7) + robot_obs (.., 15) -> the relative world-frame action (gripper_control.py:39-63): position R a, orientation
    euler(R Rr^T) - euler(tcp), wrapped to [-pi, pi], * 100, with Rr the rotation of the relative tcp-frame orientation."""
    e = robot_obs[..., 3:6]
    R = _euler_xyz(e)
    pos = (R @ action[..., :3, None])[..., 0]
    Rr = _euler_xyz(action[..., 3:6] * action.dtype.type(0.01))
    M = R @ np.swapaxes(Rr, -1, -2)
    orn = np.stack([np.arctan2(-M[..., 1, 2], M[..., 2, 2]), np.arcsin(np.clip(M[..., 0, 2], -1, 1)), np.arctan2(-M[..., 0, 1], M[..., 0, 0])], -1) - e
    orn = np.where(orn < -np.pi, orn + 2 * np.pi, orn)
    orn = np.where(orn > np.pi, orn - 2 * np.pi, orn)
    return np.concatenate([pos, (orn * 100).astype(action.dtype), action[..., 6:]], -1).astype(action.dtype)


def head(H1, W, bias):
    """-> (pre, tanh(pre), 1 - tanh(pre)^2 as 4 e / (1 + e)^2 with e = exp(-2 |pre|): exact where the prediction saturates)"""
    pre = (H1[:, None, :] * W[None, :, :]).sum(-1) + bias          # no BLAS: numpy's own pairwise sum, the same on every host (the float32 figures are tabulated)
    e = np.exp(-2 * np.abs(pre))
    return pre, np.tanh(pre), 4 * e / ((1 + e) * (1 + e))


def criterion(d, crit):
    """-> (l(d), l'(d)) per element: Huber with delta 1, or the squared error"""
    if crit == MSE:
        return d * d, 2 * d
    a = np.abs(d)
    one, half = d.dtype.type(1), d.dtype.type(0.5)
    return np.where(a <= one, half * d * d, a - half), np.where(a <= one, d, np.sign(d))


def loss(H1, W, bias, actions, robot_obs, crit, frame, grad_scale=1.0):
    """H1 (R, 2048), W (7, 2048), bias (7), actions (R, 7), robot_obs (R, 15).  frame 0: the target is the world-frame action (DeterministicDecoder.loss);
    frame 1: world_to_tcp_frame(actions, robot_obs) (loss_and_act).  -> dict: pre, p, d (R, 7); row_loss (R) = sum_j l / 7; pred (R, 7) = tcp_to_world(p);
    dpre (R, 7) = grad_scale l'(d) (1 - p^2) / 7."""
    dt = H1.dtype.type
    pre, p, dtanh = head(H1, W, bias)
    tgt = world_to_tcp(actions, robot_obs).astype(H1.dtype) if frame else actions
    d = p - tgt
    l, g = criterion(d, crit)
    return dict(pre=pre, p=p, d=d, row_loss=l.sum(-1) / dt(7), pred=tcp_to_world(p, robot_obs), dpre=dt(grad_scale) * g * dtanh / dt(7))


def bwd(dpre, W, H1, last):
    """dpre (R, 7), H1 (R, 2048); `last`: bool (R) rows of the last time step.  -> dH1 (R, 2048), dZ1 (last rows, 2048) = dH1 (H1 > 0), dW (7, 2048), db (7)"""
    dH1 = (dpre[:, :, None] * W[None, :, :]).sum(1)
    return dH1, np.where(H1[last] > 0, dH1[last], H1.dtype.type(0)), (dpre[:, :, None] * H1[:, None, :]).sum(0), dpre.sum(0)


def torch_autograd(H1, W, bias, actions, robot_obs, crit, frame, grad_scale):
    """The same quantities from torch (float64): nn.HuberLoss / nn.MSELoss with reduction "sum" scaled by grad_scale / 7 (the engine's grad_scale carries the
    1 / rows of reduction "mean"), gradients by autograd.  -> row_loss, dH1, dW, db, dpre"""
    import torch
    h = torch.from_numpy(np.asarray(H1, np.float64)).requires_grad_(True)
    w = torch.from_numpy(np.asarray(W, np.float64)).requires_grad_(True)
    b = torch.from_numpy(np.asarray(bias, np.float64)).requires_grad_(True)
    pre = h @ w.T + b
    pre.retain_grad()
    p = torch.tanh(pre)
    tgt = torch.from_numpy(world_to_tcp(np.asarray(actions, np.float64), np.asarray(robot_obs, np.float64)) if frame else np.asarray(actions, np.float64))
    fn = torch.nn.MSELoss(reduction="none") if crit == MSE else torch.nn.HuberLoss(reduction="none")
    l = fn(p, tgt)
    (l.sum() * grad_scale / 7).backward()
    return (l.sum(-1) / 7).detach().numpy(), h.grad.numpy(), w.grad.numpy(), b.grad.numpy(), pre.grad.numpy()
