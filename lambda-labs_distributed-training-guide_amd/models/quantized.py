"""Weight-only FP8 copies of a Llama-family model's decode-step matrices.

At one sequence per step the projections of a decode step stream every weight once and use it once:
`ops.skinny_linear` already reads bf16 weights at the copy rate, so the step's time is the bytes of its
weights.  `Fp8DecodeWeights` quantises those matrices once, at load time, to OCP e4m3fn with one f32 scale
per output row (`ops.quantize_fp8_rows`), and `decode_step(..., linear="skinny-fp8", fp8=...)` streams the
one-byte copies through `ops.skinny_linear_fp8`.  Activations, the KV cache, the norms and the embedding
lookup stay bf16.  The model is not modified: the FP8 copies live beside it (`nbytes` more memory, about half
of the matrices' bf16 size).  The prefill of such a run (`prefill(..., fp8=...)`) stays hipBLASLt in bf16, on
the matrices `dequantized` returns, made one at a time: were it to use the model's own weights, the prompt's
keys and values would come from another model than the decode steps that attend to them (measured on the
tiny test models: logit error 0.20-0.27 against 0.07-0.09 for either model alone).

With the default power-of-two scales float(wq) * scale is exactly representable in bf16, so the quantised
model is exactly some bf16 model: `dequantized(name)` returns that model's matrix.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import ops
from .generation import _check_model

LAYER_MATRICES = ("self_attn.qkv_proj", "self_attn.o_proj", "mlp.gate_up_proj", "mlp.down_proj")
HEAD = "lm_head"


class Fp8DecodeWeights:
    """(wq, scale) of every layer's qkv_proj, o_proj, gate_up_proj and down_proj, and with `head=True` of the
    LM head (for tied embeddings a quantised copy of the embedding matrix; the lookup itself stays bf16).
    Names are the modules' paths: "layers.0.self_attn.qkv_proj", ..., "lm_head"."""

    def __init__(self, model, head: bool = True, pow2: bool = True):
        _check_model(model)
        self.pow2 = bool(pow2)
        self.tensors: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        for i, layer in enumerate(model.layers):
            for name in LAYER_MATRICES:
                mod = layer
                for part in name.split("."):
                    mod = getattr(mod, part)
                self.tensors[f"layers.{i}.{name}"] = ops.quantize_fp8_rows(mod.weight.detach(), pow2=self.pow2)
        if head:
            self.tensors[HEAD] = ops.quantize_fp8_rows(model.lm_head_weight().detach(), pow2=self.pow2)
        self.num_layers = len(model.layers)
        self.device = model.embed_tokens.weight.device

    @property
    def has_head(self) -> bool:
        return HEAD in self.tensors

    def layer(self, i: int, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.tensors[f"layers.{i}.{name}"]

    def head(self) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.tensors[HEAD]

    def names(self):
        return list(self.tensors)

    @property
    def nbytes(self) -> int:
        """Bytes of the FP8 copies and their scales: memory held beside the model's bf16 weights."""
        return sum(wq.numel() * wq.element_size() + s.numel() * s.element_size() for wq, s in self.tensors.values())

    def dequantized(self, name: str) -> torch.Tensor:
        """float(wq) * scale as bf16 (exact for power-of-two scales)."""
        wq, scale = self.tensors[name]
        return (wq.float() * scale[:, None]).to(torch.bfloat16)

    def check(self, model):
        """The copies belong to a model of this shape on this device."""
        if self.num_layers != len(model.layers) or self.device != model.embed_tokens.weight.device:
            raise ValueError("Fp8DecodeWeights: built for another model or device")
