"""The loss the reference's trainer leaves out: trainer.py:324-331 trains on the value alone ("策略损失（简化版：
只用价值损失）/ 完整版需要把move_probs转换为target policy").  This is that full version for a `ChessNet`:

    states, target_values, target = buf.sample_policy_tensors(64, player_plane="record")
    total, value_loss, policy_loss = training.loss(net, states, target_values, target)
    total.backward()

`policy_loss` is the cross-entropy between the visit distribution pi of a position's legal moves
(self_play.py:234-239) and the softmax the search itself applies to the logits, over the legal moves only
(neural_network.py:148-169).  Forward and backward are one hand-written HIP kernel each (csrc/xq_policy_loss.hip);
the target stays sparse ([B, 128] columns and probabilities) and never visits the host.  There is no library
fallback: anything the kernels do not cover raises.
"""
import ctypes as C

import torch

from . import _lib
from .replay import PolicyTarget  # noqa: F401  (the target type, re-exported)


def _chk(rc, what):
    if rc != 0:
        raise _lib.XqError("%s failed (%d): bad argument or HIP launch error" % (what, rc))


def _check_target(target, batch):
    cols, pi, n_moves = target
    for name, t, dtype, shape in (("cols", cols, torch.int32, (batch, _lib.MAX_MOVES)),
                                  ("pi", pi, torch.float32, (batch, _lib.MAX_MOVES)),
                                  ("n_moves", n_moves, torch.int32, (batch,))):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("policy_loss: target.%s must be a contiguous %s CUDA tensor of shape %s"
                             % (name, str(dtype).replace("torch.", ""), list(shape)))


class _PolicyLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, cols, pi, n_moves):
        B, n_cols = logits.shape
        L = _lib.lib()
        loss = torch.empty((B,), dtype=torch.float32, device=logits.device)
        resid = torch.empty((B, _lib.MAX_MOVES), dtype=torch.float32, device=logits.device)
        stream = torch.cuda.current_stream().cuda_stream
        _chk(L.xq_policy_loss_f32(C.c_void_p(stream), C.c_void_p(logits.data_ptr()), logits.stride(0), n_cols,
                                  C.c_void_p(cols.data_ptr()), C.c_void_p(pi.data_ptr()),
                                  C.c_void_p(n_moves.data_ptr()), B, C.c_void_p(loss.data_ptr()),
                                  C.c_void_p(resid.data_ptr())), "xq_policy_loss_f32")
        ctx.save_for_backward(resid, cols, n_moves)
        ctx.n_cols = n_cols
        ctx.mark_non_differentiable(resid)
        return loss, resid

    @staticmethod
    def backward(ctx, grad_loss, _grad_resid):
        resid, cols, n_moves = ctx.saved_tensors
        B = resid.shape[0]
        scale = grad_loss.to(torch.float32).contiguous()
        grad = torch.empty((B, ctx.n_cols), dtype=torch.float32, device=resid.device)
        stream = torch.cuda.current_stream().cuda_stream
        _chk(_lib.lib().xq_policy_loss_grad_f32(C.c_void_p(stream), C.c_void_p(resid.data_ptr()),
                                                C.c_void_p(cols.data_ptr()), C.c_void_p(n_moves.data_ptr()),
                                                C.c_void_p(scale.data_ptr()), 0.0, B, C.c_void_p(grad.data_ptr()),
                                                grad.stride(0), ctx.n_cols), "xq_policy_loss_grad_f32")
        return grad, None, None, None


def policy_loss_rows(logits, target):
    """(loss float32 [B], resid float32 [B, 128]): the per-row losses (differentiable with respect to `logits`) and the
    sparse residual p_i - pi_i the forward kernel leaves for the backward one."""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2
            and logits.is_contiguous() and logits.shape[0] > 0 and logits.shape[1] > 0):
        raise ValueError("policy_loss: logits must be a contiguous float32 CUDA tensor [B, n_cols] (the hand-written "
                         "kernels cover nothing else and there is no library fallback)")
    _check_target(target, logits.shape[0])
    return _PolicyLoss.apply(logits, *target)


def policy_loss(logits, target, reduction="mean"):
    """Legal-move cross-entropy of `logits` (float32 CUDA [B, n_cols], contiguous: ChessNet.forward's first output, or
    a compact head's with the matching column map in the target) against a `PolicyTarget`.
    reduction: "mean" / "sum" over the rows (a torch op on the per-row losses), or "none" for the rows themselves.
    Backward writes the dense gradient [B, n_cols] in one pass, scaled per row by the incoming gradient."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError("policy_loss: reduction must be 'mean', 'sum' or 'none'")
    rows, _ = policy_loss_rows(logits, target)
    if reduction == "none":
        return rows
    return rows.mean() if reduction == "mean" else rows.sum()


def loss(network, states, target_values, target, policy_weight=1.0):
    """trainer.py:324-331 with the policy term: (total, value_loss, policy_loss) where value_loss =
    nn.MSELoss()(value, target_values) as in trainer.py:327 and total = value_loss + policy_weight * policy_loss.
    `network(states)` returns (logits, value) like ChessNet.forward; feed it states whose player plane is the real
    side to move (sample_policy_tensors(player_plane="record")): a move distribution belongs to the side that moves."""
    logits, value = network(states)
    value_loss = torch.nn.MSELoss()(value, target_values)
    p_loss = policy_loss(logits, target)
    return value_loss + policy_weight * p_loss, value_loss, p_loss
