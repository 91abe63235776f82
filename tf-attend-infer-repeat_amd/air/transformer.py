"""Spatial transformer ops -- mirror of the reference's air/transformer.py:18-195.

``transformer(U, theta, out_size)`` and ``batch_transformer(U, thetas, out_size)`` keep the reference signatures; U is
[B, H, W, C] (any C; [B, H, W] is taken as one channel and returned without the channel axis) float32 on the GPU, theta
[B, 6] or [B, 2, 3], thetas [B, T, 6] or [B, T, 2, 3].
Runs the hand-written HIP kernels; no CPU fallback.  One channel goes through air_transformer_fwd / air_transformer_bwd
(the AIR path, air_model.py:331, 364), several channels and batch_transformer through air_transformer_nc_fwd /
air_transformer_nc_bwd, which sample image b for row b*T+t without copying it T times.
When U or theta require a gradient the ops are differentiable the way the reference's are under tf.gradients (same op
order, see include/air_hip.h); torch.autograd only carries the call."""
import torch

from . import _hip as H


def _nc_forward(U, theta, out_size, T):
    """out [B*T,Ho,Wo,C] of U [B,Hi,Wi,C] under theta [B*T,6] (row b*T+t samples image b)"""
    B, Hi, Wi, Ch = (int(v) for v in U.shape)
    Ho, Wo = int(out_size[0]), int(out_size[1])
    Uc = U.contiguous().float()
    th = theta.reshape(B * T, 6).contiguous().float()
    out = torch.empty(B * T, Ho, Wo, Ch, dtype=torch.float32, device=U.device)
    H.launch("air_transformer_nc_fwd", U.device, H.ptr(Uc), H.ptr(th), H.ptr(out), B, T, Hi, Wi, Ch, Ho, Wo)
    return out


def _nc_grad(U, theta, out_size, d_out, T, need_dU, need_dtheta):
    B, Hi, Wi, Ch = (int(v) for v in U.shape)
    Ho, Wo = int(out_size[0]), int(out_size[1])
    Uc = U.contiguous().float()
    th = theta.reshape(B * T, 6).contiguous().float()
    g = d_out.reshape(B * T, Ho, Wo, Ch).contiguous().float()
    dU = torch.empty_like(Uc) if need_dU else None
    dth = torch.empty_like(th) if need_dtheta else None
    H.launch("air_transformer_nc_bwd", U.device, H.ptr(Uc), H.ptr(th), H.ptr(g), H.ptr(dU), H.ptr(dth), B, T, Hi, Wi, Ch, Ho, Wo)
    return dU, dth


def transformer_grad(U, theta, out_size, d_out, need_dU=True, need_dtheta=True):
    """(d_U [B,Hi,Wi], d_theta [B,6]) of transformer(U, theta, out_size) for an incoming d_out [B,Ho,Wo]; with a
    [B,Hi,Wi,C] input of C > 1 channels, d_U [B,Hi,Wi,C] for d_out [B,Ho,Wo,C]."""
    if U.dim() == 4 and U.shape[3] != 1:
        return _nc_grad(U, theta, out_size, d_out, 1, need_dU, need_dtheta)
    B, Hi, Wi = int(U.shape[0]), int(U.shape[1]), int(U.shape[2])
    Ho, Wo = int(out_size[0]), int(out_size[1])
    Uc = U.reshape(B, Hi, Wi).contiguous().float()
    th = theta.reshape(B, 6).contiguous().float()
    g = d_out.reshape(B, Ho, Wo).contiguous().float()
    dU = torch.empty_like(Uc) if need_dU else None
    dth = torch.empty_like(th) if need_dtheta else None
    H.launch("air_transformer_bwd", U.device, H.ptr(Uc), H.ptr(th), H.ptr(g), H.ptr(dU), H.ptr(dth), B, Hi, Wi, Ho, Wo)
    return dU, dth


def batch_transformer_grad(U, thetas, out_size, d_out, need_dU=True, need_dtheta=True):
    """(d_U [B,Hi,Wi,C], d_thetas [B*T,6]) of batch_transformer(U, thetas, out_size) for an incoming d_out [B*T,Ho,Wo,C]
    (a 3-D U: d_U [B,Hi,Wi], d_out [B*T,Ho,Wo]).  d_U[b] is the sum of its T rows' gradients in ascending t."""
    T = int(thetas.shape[1])
    U4 = U.unsqueeze(3) if U.dim() == 3 else U
    dU, dth = _nc_grad(U4, thetas, out_size, d_out, T, need_dU, need_dtheta)
    return (dU.reshape(U.shape) if dU is not None else None), dth


class _TransformerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, theta, out_size):
        ctx.save_for_backward(U, theta)
        ctx.out_size = out_size
        return transformer(U.detach(), theta.detach(), out_size)

    @staticmethod
    def backward(ctx, d_out):
        U, theta = ctx.saved_tensors
        dU, dth = transformer_grad(U, theta, ctx.out_size, d_out, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (dU.reshape(U.shape) if dU is not None else None,
                dth.reshape(theta.shape) if dth is not None else None, None)


class _BatchTransformerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, thetas, out_size):
        ctx.save_for_backward(U, thetas)
        ctx.out_size = out_size
        return batch_transformer(U.detach(), thetas.detach(), out_size)

    @staticmethod
    def backward(ctx, d_out):
        U, thetas = ctx.saved_tensors
        dU, dth = batch_transformer_grad(U, thetas, ctx.out_size, d_out, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return dU, (dth.reshape(thetas.shape) if dth is not None else None), None


def transformer(U, theta, out_size, name="SpatialTransformer", **kwargs):
    if torch.is_grad_enabled() and (U.requires_grad or theta.requires_grad):
        return _TransformerFn.apply(U, theta, tuple(out_size))
    H.require_device(U, "U", "transformer")
    squeeze = U.dim() == 4
    if squeeze and U.shape[3] != 1:
        return _nc_forward(U, theta, out_size, 1)
    B, Hi, Wi = int(U.shape[0]), int(U.shape[1]), int(U.shape[2])
    Ho, Wo = int(out_size[0]), int(out_size[1])
    Uc = U.reshape(B, Hi, Wi).contiguous().float()
    th = theta.reshape(B, 6).contiguous().float()
    out = torch.empty(B, Ho, Wo, dtype=torch.float32, device=U.device)
    H.launch("air_transformer_fwd", U.device, H.ptr(Uc), H.ptr(th), H.ptr(out), B, Hi, Wi, Ho, Wo)
    return out.unsqueeze(3) if squeeze else out


def batch_transformer(U, thetas, out_size, name="BatchSpatialTransformer"):
    """transformer.py:178-195: thetas [B,T,6] (or [B,T,2,3]) holds T transforms per input; returns [B*T,Ho,Wo,C], row b*T+t
    being input b under thetas[b,t] ([B*T,Ho,Wo] for a 3-D U)."""
    if torch.is_grad_enabled() and (U.requires_grad or thetas.requires_grad):
        return _BatchTransformerFn.apply(U, thetas, tuple(out_size))
    H.require_device(U, "U", "batch_transformer")
    out = _nc_forward(U.unsqueeze(3) if U.dim() == 3 else U, thetas, out_size, int(thetas.shape[1]))
    return out.squeeze(3) if U.dim() == 3 else out
