"""The batched solve as a differentiable torch operation: forces = solve(records, costs), its
backward pass one call of ``BatchSolver.sensitivity`` (the fp64 Riccati adjoint of
``cmpc_batch_sensitivity``, include/cmpc_solver.h). float32 at the tensor boundary; the fp64
gradients are cast.
"""
from __future__ import annotations

import torch

from .records import (COST_ALPHA, COST_WEIGHTS, COST_WORDS, REC_HDR, REC_P, REC_V, REC_W, SENS_ALPHA,
                      SENS_WEIGHTS, SENS_WORDS, SENS_X0)


def _ordered(solver, device):
    """The handle's stream as a torch stream, ordered after torch's current one."""
    s = torch.cuda.ExternalStream(solver.stream_handle, device=device)
    s.wait_stream(torch.cuda.current_stream(device))
    return s


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, solver, records, costs, act_tol):
        B, N = records.shape[0], solver.horizon
        records = records.contiguous()
        if costs is not None:
            solver.set_instance_costs(costs.detach().contiguous())
        forces = torch.empty((B, 12 * N), dtype=torch.float32, device=records.device)
        status = torch.empty(B, dtype=torch.uint8, device=records.device)
        s = _ordered(solver, records.device)
        solver.solve(records.detach(), forces, status)
        torch.cuda.current_stream(records.device).wait_stream(s)
        ctx.solver, ctx.act_tol, ctx.has_costs = solver, act_tol, costs is not None
        ctx.save_for_backward(records.detach(), forces)
        ctx.mark_non_differentiable(status)
        return forces, status

    @staticmethod
    def backward(ctx, grad_forces, _grad_status):
        records, forces = ctx.saved_tensors
        solver = ctx.solver
        B, N = records.shape[0], solver.horizon
        dev = records.device
        v = grad_forces.to(torch.float32).contiguous()
        sens = torch.empty((B, SENS_WORDS), dtype=torch.float64, device=dev)
        dtraj = torch.empty((B, 12 * N), dtype=torch.float64, device=dev)
        s = _ordered(solver, dev)
        solver.sensitivity(records, forces, v, sens, dtraj=dtraj, act_tol=ctx.act_tol)
        torch.cuda.current_stream(dev).wait_stream(s)
        g_rec = torch.zeros_like(records)
        # dL/dx_0 is in the order of the traj rows (rpy, p, w, v); rpy has no record word
        g_rec[:, REC_P:REC_P + 3] = sens[:, SENS_X0 + 3:SENS_X0 + 6].to(torch.float32)
        g_rec[:, REC_W:REC_W + 3] = sens[:, SENS_X0 + 6:SENS_X0 + 9].to(torch.float32)
        g_rec[:, REC_V:REC_V + 3] = sens[:, SENS_X0 + 9:SENS_X0 + 12].to(torch.float32)
        g_rec[:, REC_HDR:REC_HDR + 12 * N] = dtraj.to(torch.float32)
        g_cost = None
        if ctx.has_costs:
            g_cost = torch.zeros((B, COST_WORDS), dtype=torch.float32, device=dev)
            g_cost[:, COST_WEIGHTS:COST_WEIGHTS + 12] = sens[:, SENS_WEIGHTS:SENS_WEIGHTS + 12].to(torch.float32)
            g_cost[:, COST_ALPHA] = sens[:, SENS_ALPHA].to(torch.float32)
        return None, g_rec, g_cost, None


def differentiable_solve(solver, records, costs=None, act_tol: float = 1e-3):
    """``solver.solve`` of ``records`` [B, record words] float32 on the device, differentiable ->
    (forces [B, 12N] float32, status [B] uint8; the status is not differentiable).

    ``costs`` [B, 16] float32 (rows as ``make_instance_costs`` builds them), when given, becomes the
    handle's cost table (``set_instance_costs``) before the solve and stays in force after it.

    The backward pass calls ``solver.sensitivity`` once, at the solved forces, with rows active up
    to ``act_tol`` newtons. The gradient with respect to ``records`` has the body position p,
    velocity v, angular velocity w and the trajectory words filled (``SENS_X0`` and ``dtraj`` cast
    to float32); every other word is zero: the derivative through the quaternion, the foot offsets,
    x_drag, f_est(3) and the gait is not propagated. The partial derivative with respect to x_0's
    roll, pitch and yaw at a fixed rotation matrix has no record word: take it from words
    ``SENS_X0 .. SENS_X0 + 2`` of a direct ``solver.sensitivity`` call. With ``costs`` the gradient
    with respect to it is [B, 16]: the twelve weights, alpha, zeros. An instance that failed (a
    non-zero status, zero forces) gets zero gradients. What the gradients are at a weakly active
    constraint: include/cmpc_solver.h, cmpc_batch_sensitivity."""
    return _Solve.apply(solver, records, costs, act_tol)
