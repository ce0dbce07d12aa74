"""Torch side shared by the fused recurrent layers (lstm.py, gru.py,
lstm_multi.py): batch padding to the kernels' 64-row tile, the forward
launch, and the W_hh / b_hh gradients.

Layouts are (T, B, ·) for one model and (M, T, B, ·) for a stack of M; the
helpers take whatever leads the (T, B) axes as it comes.
"""

from __future__ import annotations

import torch

BATCH_TILE = 64              # rows per block of the recurrent kernels


def pad_batch(x: torch.Tensor, dim: int):
    """Zero-pad the batch axis `dim` to a multiple of the kernel tile.

    Returns (padded x, unpad); unpad(h) cuts the same axis of a result back
    to the original batch (and is the identity when nothing was padded).
    """
    B = x.shape[dim]
    pad = (-B) % BATCH_TILE
    if not pad:
        return x, lambda h: h
    shape = list(x.shape)
    shape[dim] = pad
    return (torch.cat([x, x.new_zeros(shape)], dim=dim),
            lambda h: h.narrow(dim, 0, B))


def launch_fwd(binding, xproj: torch.Tensor, w_hh: torch.Tensor,
               b_hh: torch.Tensor, n_gates: int, save: bool):
    """One fused forward launch over xproj (..., T, B, G*H) bf16.

    f32 master W_hh (..., H, G*H) and b_hh (..., G*H) enter the kernel as
    bf16 W_hh^T and f32 bias. save=True is the training launch: returns
    (h_out, gates, aux, w_bf) with the kernel's backward saves (aux is c for
    the LSTM, hp_n for the GRU) and the bf16 W_hh the backward kernel reads.
    save=False is the serving launch: null save pointers, ~5x fewer global
    writes per cell, returns h_out alone.
    """
    assert xproj.dtype == torch.bfloat16 and xproj.is_cuda
    *lead, T, B, GH = xproj.shape
    H = GH // n_gates
    dev = xproj.device
    w_bf = w_hh.detach().to(torch.bfloat16).contiguous()      # (.., H, G*H)
    wt_bf = w_bf.transpose(-1, -2).contiguous()               # (.., G*H, H)
    bias = b_hh.detach().float().contiguous()
    xproj = xproj.contiguous()
    h_out = torch.empty((*lead, T, B, H), dtype=torch.bfloat16, device=dev)
    gates = aux = None
    if save:
        gates = torch.empty((*lead, T, B, GH), dtype=torch.bfloat16,
                            device=dev)
        aux = torch.empty((*lead, T, B, H), dtype=torch.float32, device=dev)
    binding(xproj.data_ptr(), wt_bf.data_ptr(), bias.data_ptr(),
            h_out.data_ptr(), gates.data_ptr() if save else 0,
            aux.data_ptr() if save else 0, *lead, B, T, H, int(save),
            torch.cuda.current_stream(dev).cuda_stream)
    return (h_out, gates, aux, w_bf) if save else h_out


def hh_grads(h_out: torch.Tensor, dg: torch.Tensor, time_dim: int):
    """(dW_hh, db_hh) from the saved sequence h_out (..., T, B, H) and the
    h-side pre-activation grads dg (..., T, B, G*H), both bf16.

    dW_hh = sum_t h_{t-1}^T dg_t with h_{-1} = 0: one bf16 GEMM per model
    (mm, or bmm for a stack) with f32 accumulation inside and a bf16 result
    (torch.autocast semantics; no f32 copy of dg), then cast to f32. db_hh
    is the f32 sum of dg over (T, B).
    """
    T = h_out.shape[time_dim]
    first = list(h_out.shape)
    first[time_dim] = 1
    h_prev = torch.cat([h_out.new_zeros(first),
                        h_out.narrow(time_dim, 0, T - 1)], dim=time_dim)
    lead = h_out.shape[:time_dim]
    dg = dg.reshape(*lead, -1, dg.shape[-1])                  # (.., T*B, G*H)
    h_prev = h_prev.reshape(*lead, -1, h_out.shape[-1])       # (.., T*B, H)
    return ((h_prev.transpose(-1, -2) @ dg).float(),
            dg.sum(dim=-2, dtype=torch.float32))
