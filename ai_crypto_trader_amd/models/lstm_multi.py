"""M independent LSTM price predictors trained and served as one stacked
pass.

NeuralNetworkService keeps one LSTMPricePredictor per symbol. At the
service batch size (32, padded to 64 rows) a single model's fused
recurrence is one block on a 256-CU part, followed by a handful of tiny
GEMMs and an Adam step — repeated per symbol. Here the M models' parameters
are stacked along a leading model axis: the recurrence runs as one
(B/64, M)-block launch of the same kernels (ops/hip/lstm.hip, blockIdx.y =
model, each block staging only its own model's W_hh), and everything
around it is a batched GEMM (torch.bmm) over the stacked parameters.

The models stay independent: no parameter is shared, model i's outputs and
gradients depend only on slab i, and Adam is element-wise, so one Adam over
the stacked parameters is the arithmetic of M separate Adams.
`from_models` / `export_model` convert to and from ordinary
LSTMPricePredictors, so checkpoints are interchangeable.

On CPU the stacked layers run the f32 time loop (`_forward_reference`); on
a GPU machine the HIP path is mandatory (ops.require_hip_ops).
"""

from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import require_hip_ops
from ._recurrent import hh_grads, launch_fwd, pad_batch
from .lstm import LSTMPricePredictor


class _FusedLSTMSeqMulti(torch.autograd.Function):
    """Recurrent part only: xproj (M,T,B,4H) bf16 -> h_out (M,T,B,H) bf16.

    Same dtypes and operand order as lstm._FusedLSTMSeq, per model: f32
    master W_hh cast to bf16, dW_hh as one bf16 batched GEMM over the
    saved sequence, db_hh as an f32 sum.
    """

    @staticmethod
    def forward(ctx, xproj: torch.Tensor, w_hh: torch.Tensor,
                b_hh: torch.Tensor):
        h_out, gates, c_sav, w_bf = launch_fwd(
            require_hip_ops().lstm_seq_fwd_multi, xproj, w_hh, b_hh, 4,
            save=True)
        ctx.save_for_backward(gates, c_sav, h_out, w_bf)
        return h_out

    @staticmethod
    def backward(ctx, grad_h: torch.Tensor):
        gates, c_sav, h_out, w_bf = ctx.saved_tensors
        M, T, B, H = h_out.shape
        dev = grad_h.device
        dgates = torch.empty_like(gates)
        dh_up = grad_h.float().contiguous()
        require_hip_ops().lstm_seq_bwd_multi(
            dh_up.data_ptr(), gates.data_ptr(), c_sav.data_ptr(),
            w_bf.data_ptr(), dgates.data_ptr(), M, B, T, H,
            torch.cuda.current_stream(dev).cuda_stream,
        )
        return (dgates, *hh_grads(h_out, dgates, time_dim=1))


def lstm_seq_infer_multi(xproj: torch.Tensor, w_hh: torch.Tensor,
                         b_hh: torch.Tensor) -> torch.Tensor:
    """Inference-only stacked forward: no backward saves (gates/c)."""
    return launch_fwd(require_hip_ops().lstm_seq_fwd_multi, xproj, w_hh,
                      b_hh, 4, save=False)


class StackedLSTMLayer(nn.Module):
    """M independent LSTM layers: batched input projection + one fused
    multi-model recurrence launch.

    Input (M, T, B, F), output (M, T, B, H): model-major, each model's
    slab in FusedLSTMLayer's time-major layout.
    """

    def __init__(self, n_models: int, input_size: int, hidden_size: int):
        super().__init__()
        assert n_models >= 1
        assert hidden_size in (32, 64), "HIP kernel supports H in {32, 64}"
        self.n_models = n_models
        self.input_size = input_size
        self.hidden_size = hidden_size
        M, H4 = n_models, 4 * hidden_size
        self.w_ih = nn.Parameter(torch.empty(M, input_size, H4))
        self.b_ih = nn.Parameter(torch.zeros(M, H4))
        self.w_hh = nn.Parameter(torch.empty(M, hidden_size, H4))
        self.b_hh = nn.Parameter(torch.zeros(M, H4))
        k = hidden_size ** -0.5
        nn.init.uniform_(self.w_ih, -k, k)
        nn.init.uniform_(self.w_hh, -k, k)

    def forward(self, x: torch.Tensor) -> torch.Tensor:   # (M, T, B, F)
        if x.is_cuda:
            x, unpad = pad_batch(x, 2)
            M, T, Bp, F = x.shape
            bf = torch.bfloat16
            xproj = (torch.bmm(x.to(bf).reshape(M, T * Bp, F),
                               self.w_ih.to(bf))
                     + self.b_ih.to(bf)[:, None, :]).view(M, T, Bp, -1)
            if torch.is_grad_enabled():
                h = _FusedLSTMSeqMulti.apply(xproj, self.w_hh, self.b_hh)
            else:   # serving path: no backward saves
                h = lstm_seq_infer_multi(xproj, self.w_hh, self.b_hh)
            return unpad(h)
        return self._forward_reference(x)

    def _forward_reference(self, x: torch.Tensor) -> torch.Tensor:
        """Plain fp32 reference (CPU path and GPU numerics tests):
        FusedLSTMLayer._forward_reference with every matmul a bmm."""
        M, T, B, _ = x.shape
        H = self.hidden_size
        h = x.new_zeros(M, B, H)
        c = x.new_zeros(M, B, H)
        b_ih = self.b_ih[:, None, :]
        b_hh = self.b_hh[:, None, :]
        outs = []
        for t in range(T):
            g = (torch.bmm(x[:, t], self.w_ih) + b_ih
                 + torch.bmm(h, self.w_hh) + b_hh)
            i, f, gg, o = g.split(H, dim=2)
            i, f, o = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o)
            gg = torch.tanh(gg)
            c = f * c + i * gg
            h = o * torch.tanh(c)
            outs.append(h)
        return torch.stack(outs, dim=1)


# single-model state_dict key -> (stacked attribute path, transpose?)
# nn.Linear stores (out, in); the stacked head keeps (in, out) for bmm.
_KEY_MAP = {
    "l1.w_ih": ("l1.w_ih", False), "l1.b_ih": ("l1.b_ih", False),
    "l1.w_hh": ("l1.w_hh", False), "l1.b_hh": ("l1.b_hh", False),
    "l2.w_ih": ("l2.w_ih", False), "l2.b_ih": ("l2.b_ih", False),
    "l2.w_hh": ("l2.w_hh", False), "l2.b_hh": ("l2.b_hh", False),
    "head.0.weight": ("head_w1", True), "head.0.bias": ("head_b1", False),
    "head.2.weight": ("head_w2", True), "head.2.bias": ("head_b2", False),
}


class StackedLSTMPricePredictor(nn.Module):
    """M independent LSTM(64) -> LSTM(32) -> Dense(16) -> Dense(1)
    predictors: (M, B, T, F) feature windows -> (M, B) predictions."""

    HEAD = 16

    def __init__(self, n_models: int, n_features: int = 9,
                 seq_len: int = 60, hidden: tuple[int, int] = (64, 32)):
        super().__init__()
        self.n_models = n_models
        self.n_features = n_features
        self.seq_len = seq_len
        self.hidden = tuple(hidden)
        M, H2, D = n_models, hidden[1], self.HEAD
        self.l1 = StackedLSTMLayer(M, n_features, hidden[0])
        self.l2 = StackedLSTMLayer(M, hidden[0], hidden[1])
        self.head_w1 = nn.Parameter(torch.empty(M, H2, D))
        self.head_b1 = nn.Parameter(torch.empty(M, D))
        self.head_w2 = nn.Parameter(torch.empty(M, D, 1))
        self.head_b2 = nn.Parameter(torch.empty(M, 1))
        for w, b, fan_in in ((self.head_w1, self.head_b1, H2),
                             (self.head_w2, self.head_b2, D)):
            k = fan_in ** -0.5           # nn.Linear's default range
            nn.init.uniform_(w, -k, k)
            nn.init.uniform_(b, -k, k)

    def forward(self, x: torch.Tensor) -> torch.Tensor:   # (M, B, T, F)
        x = x.transpose(1, 2)                             # (M, T, B, F)
        h = self.l2(self.l1(x))
        last = h[:, -1].float()                           # (M, B, H2)
        z = torch.relu(torch.baddbmm(self.head_b1[:, None, :], last,
                                     self.head_w1))
        out = torch.baddbmm(self.head_b2[:, None, :], z, self.head_w2)
        return out.squeeze(-1)                            # (M, B)

    # --- conversion to / from single models ------------------------------
    def _slot(self, key: str) -> tuple[torch.Tensor, bool]:
        path, transpose = _KEY_MAP[key]
        obj = self
        for part in path.split("."):
            obj = getattr(obj, part)
        return obj, transpose

    @classmethod
    def from_models(cls, models: list[LSTMPricePredictor]
                    ) -> "StackedLSTMPricePredictor":
        """Stack single models (all of one architecture) into one module
        on the first model's device."""
        assert len(models) >= 1
        m0 = models[0]
        hidden = (m0.l1.hidden_size, m0.l2.hidden_size)
        stacked = cls(len(models), m0.l1.input_size, m0.seq_len, hidden)
        stacked.to(m0.l1.w_ih.device)
        for i, m in enumerate(models):
            stacked.load_model(i, m.state_dict())
        return stacked

    @torch.no_grad()
    def load_model(self, i: int, state_dict: dict) -> None:
        """Load one single-model state_dict into model slot i."""
        missing = set(_KEY_MAP) - set(state_dict)
        extra = set(state_dict) - set(_KEY_MAP)
        if missing or extra:
            raise KeyError(f"state_dict mismatch: missing {sorted(missing)}"
                           f", unexpected {sorted(extra)}")
        for key in _KEY_MAP:
            dst, transpose = self._slot(key)
            src = state_dict[key]
            dst[i].copy_(src.t() if transpose else src)

    @torch.no_grad()
    def model_state_dict(self, i: int) -> dict:
        """Model i's parameters under the single model's keys and shapes."""
        out = {}
        for key in _KEY_MAP:
            src, transpose = self._slot(key)
            v = src[i].detach()
            out[key] = (v.t() if transpose else v).clone().contiguous()
        return out

    def export_model(self, i: int) -> LSTMPricePredictor:
        """Model i as an ordinary LSTMPricePredictor (a copy)."""
        m = LSTMPricePredictor(self.n_features, self.seq_len, self.hidden)
        m.to(self.head_w1.device)
        m.load_state_dict(self.model_state_dict(i))
        return m

    # --- per-model freeze (early stopping under one shared optimizer) -----
    @torch.no_grad()
    def snapshot_model(self, i: int) -> list[torch.Tensor]:
        return [p[i].clone() for p in self.parameters()]

    @torch.no_grad()
    def restore_model(self, i: int, snap: list[torch.Tensor]) -> None:
        for p, s in zip(self.parameters(), snap):
            p[i].copy_(s)
