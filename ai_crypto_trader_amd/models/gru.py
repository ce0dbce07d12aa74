"""GRU layer on the fused gfx950 sequence kernels (ops/hip/gru.hip) —
sibling of models/lstm.py (neural_network_service.py:202-211 GRU model)."""

from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import require_hip_ops
from ._recurrent import hh_grads, launch_fwd, pad_batch


class _FusedGRUSeq(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xproj: torch.Tensor, w_hh: torch.Tensor,
                b_hh: torch.Tensor):
        h_out, gates, hpn, w_bf = launch_fwd(
            require_hip_ops().gru_seq_fwd, xproj, w_hh, b_hh, 3, save=True)
        ctx.save_for_backward(gates, hpn, h_out, w_bf)
        return h_out

    @staticmethod
    def backward(ctx, grad_h: torch.Tensor):
        gates, hpn, h_out, w_bf = ctx.saved_tensors
        T, B, H = h_out.shape
        dev = grad_h.device
        dgates_x = torch.empty_like(gates)
        dh_up = grad_h.float().contiguous()
        require_hip_ops().gru_seq_bwd(
            dh_up.data_ptr(), gates.data_ptr(), hpn.data_ptr(),
            h_out.data_ptr(), w_bf.data_ptr(), dgates_x.data_ptr(), B, T, H,
            torch.cuda.current_stream(dev).cuda_stream,
        )
        # h-side dgates: the n-column is da_n * r (gru.hip header), in bf16
        dg_h = dgates_x.clone()
        dg_h[..., 2 * H:] = dg_h[..., 2 * H:] * gates[..., :H]
        return (dgates_x, *hh_grads(h_out, dg_h, time_dim=0))


def gru_seq_infer(xproj: torch.Tensor, w_hh: torch.Tensor,
                  b_hh: torch.Tensor) -> torch.Tensor:
    """Inference-only fused forward (no backward saves): the serving path."""
    return launch_fwd(require_hip_ops().gru_seq_fwd, xproj, w_hh, b_hh, 3,
                      save=False)


class FusedGRULayer(nn.Module):
    """One GRU layer (T, B, F) -> (T, B, H); HIP path on GPU, plain fp32
    reference on CPU (also the numerics oracle for GPU tests)."""

    def __init__(self, input_size: int, hidden_size: int):
        super().__init__()
        assert hidden_size in (32, 64)
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.w_ih = nn.Parameter(torch.empty(input_size, 3 * hidden_size))
        self.b_ih = nn.Parameter(torch.zeros(3 * hidden_size))
        self.w_hh = nn.Parameter(torch.empty(hidden_size, 3 * hidden_size))
        self.b_hh = nn.Parameter(torch.zeros(3 * hidden_size))
        k = hidden_size ** -0.5
        nn.init.uniform_(self.w_ih, -k, k)
        nn.init.uniform_(self.w_hh, -k, k)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda:
            x, unpad = pad_batch(x, 1)
            bf = torch.bfloat16    # f32 master weights, bf16 GEMMs
            xproj = (x.to(bf) @ self.w_ih.to(bf) + self.b_ih.to(bf))
            if torch.is_grad_enabled():
                h = _FusedGRUSeq.apply(xproj, self.w_hh, self.b_hh)
            else:    # serving path: no backward saves
                h = gru_seq_infer(xproj, self.w_hh, self.b_hh)
            return unpad(h)
        return self._forward_reference(x)

    def _forward_reference(self, x: torch.Tensor) -> torch.Tensor:
        T, B, _ = x.shape
        H = self.hidden_size
        h = x.new_zeros(B, H)
        outs = []
        for t in range(T):
            xp = x[t] @ self.w_ih + self.b_ih
            hp = h @ self.w_hh + self.b_hh
            xr, xz, xn = xp.split(H, dim=1)
            hr, hz, hn = hp.split(H, dim=1)
            r = torch.sigmoid(xr + hr)
            z = torch.sigmoid(xz + hz)
            n = torch.tanh(xn + r * hn)
            h = (1 - z) * n + z * h
            outs.append(h)
        return torch.stack(outs, dim=0)
