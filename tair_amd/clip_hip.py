"""OpenCLIP ViT-H/14 text tower on the HIP kernels (reference: terediff/model/clip.py:8-61,
open_clip/transformer.py:199-256; the stock-torch form is tair_amd/clip.py).

Opt-in (``ControlLDM(..., clip_backend="hip")``): stage 3 re-encodes the prompt after every sampler step, so
the tower is per-step work there, and its 23 identical width-1024 blocks with 16 heads of d = 64 are the shapes
the GEMM and attention kernels were built for.  Driven from Python over the kernel ABI (include/tair_kernels.h),
as vae_hip.py drives the VAE:

* weights packed to bf16 once ([N][K] K-major rows, the GEMM's layout), biases / LayerNorm parameters / the
  embedding tables fp32;
* the residual stream is carried as two bf16 planes, hi = bf16(x) and lo = bf16(x - hi), side by side in one
  [T, 2C] buffer (x to ~2^-16): written by tair_k_embed_tokens and by the out-proj / c_proj GEMMs (``out_lo``),
  read by the same GEMMs' residual (``res_lo``) and by tair_k_layernorm_split;
* per block, 7 launches: ln_1 -> q|k|v GEMM -> tair_k_attention_causal (q, k, v strided out of the fused
  [T, 3C] buffer) -> out-proj GEMM (+ residual, in place) -> ln_2 -> c_fc GEMM (GELU epilogue, act 3) ->
  c_proj GEMM (+ residual, in place); then ln_final with fp32 output.  1 + 7 n + 1 launches for n blocks
  (``layer="penultimate"``: n = layers - 1).

After construction a forward allocates nothing but the tensor it returns (workspaces are sized for
``max_batch``) and never synchronises with the host, so testr.GraphedTextEncoder captures and replays it like
the stock tower.  A missing kernel or a refused plan raises ``TairError``: there is no fallback to torch.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Union

import torch
import torch.nn as nn

from . import _lib
from .clip import CONTEXT, BPETokenizer, FrozenOpenCLIPEmbedder, tokenize

LN_EPS = 1e-5
_BLK = "model.transformer.resblocks."
# packed name -> (reference key inside a block, packed dtype)
_BLOCK_KEYS = {
    "w_qkv": ("attn.in_proj_weight", torch.bfloat16), "b_qkv": ("attn.in_proj_bias", torch.float32),
    "w_out": ("attn.out_proj.weight", torch.bfloat16), "b_out": ("attn.out_proj.bias", torch.float32),
    "w_fc": ("mlp.c_fc.weight", torch.bfloat16), "b_fc": ("mlp.c_fc.bias", torch.float32),
    "w_proj": ("mlp.c_proj.weight", torch.bfloat16), "b_proj": ("mlp.c_proj.bias", torch.float32),
    "g_ln1": ("ln_1.weight", torch.float32), "b_ln1": ("ln_1.bias", torch.float32),
    "g_ln2": ("ln_2.weight", torch.float32), "b_ln2": ("ln_2.bias", torch.float32),
}
_TOP_KEYS = {
    "tok": "model.token_embedding.weight", "pos": "model.positional_embedding",
    "g_lnf": "model.ln_final.weight", "b_lnf": "model.ln_final.bias",
}
# reference parameters the forward never reads (clip.py:37-44 stops at ln_final)
_UNUSED = ("model.text_projection", "model.logit_scale")


def count_layers(sd: Dict[str, torch.Tensor]) -> int:
    n = 0
    while f"{_BLK}{n}.ln_1.weight" in sd:
        n += 1
    return n


def pack_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Reference-key state dict of a FrozenOpenCLIPEmbedder -> the packed tensors of HipTextTower: per-block
    tensors stacked over the blocks, linear weights as bf16 [N][K] rows (nn.Linear's own layout: K-major),
    everything else fp32."""
    n = count_layers(sd)
    if n < 1:
        raise _lib.TairError("clip_hip: no model.transformer.resblocks.* keys in the state dict")
    out = {name: sd[key].detach().float().contiguous() for name, key in _TOP_KEYS.items()}
    for name, (key, dt) in _BLOCK_KEYS.items():
        out[name] = torch.stack([sd[f"{_BLK}{i}.{key}"].detach().float().to(dt) for i in range(n)]).contiguous()
    return out


def unpack_state_dict(packed: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of pack_state_dict: reference key names, the linear weights as the bf16 values the kernels
    read, everything else the fp32 values that were packed."""
    out = {key: packed[name] for name, key in _TOP_KEYS.items()}
    for name, (key, _) in _BLOCK_KEYS.items():
        for i in range(packed[name].shape[0]):
            out[f"{_BLK}{i}.{key}"] = packed[name][i]
    return out


def _r64(n: int) -> int:
    return (n + 63) // 64 * 64


class _Tables(nn.Module):
    """``tower.model``: the attribute path of the reference's positional embedding (val.py / pipeline read
    ``model.clip.model.positional_embedding`` for the context length and device)."""

    def __init__(self, pos: torch.Tensor):
        super().__init__()
        self.positional_embedding = nn.Parameter(pos, requires_grad=False)


class HipTextTower(nn.Module):
    """FrozenOpenCLIPEmbedder on the HIP kernels: same ``forward(tokens)`` / ``encode(text)``, fp32 [B, L, C]."""

    def __init__(self, src: Union[FrozenOpenCLIPEmbedder, Dict[str, torch.Tensor]], *, layer: Optional[str] = None,
                 max_batch: int = 8, device="cuda", bpe_path: Optional[str] = None):
        super().__init__()
        if isinstance(src, nn.Module):
            sd = src.state_dict()
            layer = layer or ("last" if src.layer_idx == 0 else "penultimate")
            tok = src._tok
        else:
            sd, tok = src, None
        layer = layer or "penultimate"
        if layer not in ("last", "penultimate"):
            raise NotImplementedError(layer)
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.TairError("tair_amd.HipTextTower needs a ROCm GPU (no CPU fallback)")
        self.layer_idx = 0 if layer == "last" else 1
        self._tok = BPETokenizer(bpe_path) if bpe_path else tok
        self.max_batch = int(max_batch)
        self._L = _lib.lib()
        self._plans: Dict[tuple, List] = {}
        self._set_packed(pack_state_dict(sd), dev)

    # ------------------------------------------------------------------ weights
    def _set_packed(self, packed: Dict[str, torch.Tensor], dev):
        pos = packed["pos"]
        self.ctx, self.width = int(pos.shape[0]), int(pos.shape[1])
        self.layers = int(packed["w_qkv"].shape[0])
        C = self.width
        if C % 64 or self.ctx > 128 or self.layers - self.layer_idx < 0:
            raise _lib.TairError(f"HipTextTower: width {C} (heads of 64 channels), context {self.ctx} (<= 128)")
        self.heads = C // 64
        self.vocab = int(packed["tok"].shape[0])
        self.model = _Tables(pos.to(dev))
        for name, t in packed.items():
            if name != "pos":
                self.register_buffer(name, t.to(dev).contiguous())
        T = self.max_batch * self.ctx
        bf = dict(dtype=torch.bfloat16, device=dev)
        # workspaces (never reallocated: a captured graph keeps pointing at them)
        self._xs = torch.zeros((T, 2 * C), **bf)   # residual stream, planes hi | lo
        self._y = torch.zeros((T, C), **bf)        # LayerNorm output
        self._qkv = torch.zeros((T, 3 * C), **bf)
        self._ao = torch.zeros((T, C), **bf)
        self._h = torch.zeros((T, 4 * C), **bf)
        self._out = torch.zeros((self.max_batch, self.ctx, C), dtype=torch.float32, device=dev)
        self._part = torch.empty(6 * _r64(T) * 4 * C, dtype=torch.float32, device=dev)  # split-K slabs
        self._sem = torch.zeros(max(16384, 32 * (_r64(T) // 64) * (4 * C // 64)), dtype=torch.int32, device=dev)
        self._plans.clear()

    def reference_keys(self) -> set:
        """The reference (FrozenOpenCLIPEmbedder) parameter names this tower is packed from."""
        keys = set(_TOP_KEYS.values())
        for key, _ in _BLOCK_KEYS.values():
            keys.update(f"{_BLK}{i}.{key}" for i in range(self.layers))
        return keys

    def load_state_dict(self, sd, strict: bool = True, **kw):
        """Reference key names (``model.token_embedding.weight`` ...: a checkpoint's ``clip.*`` keys) are repacked
        for the kernels; the tower's own (packed) state dict loads as any module's."""
        if _TOP_KEYS["tok"] not in sd:
            return super().load_state_dict(sd, strict=strict, **kw)
        want = self.reference_keys()
        missing = sorted(want - set(sd))
        unexpected = sorted(k for k in sd if k not in want and k not in _UNUSED)
        if strict and (missing or unexpected):
            raise RuntimeError(f"HipTextTower.load_state_dict: missing {missing[:5]} ({len(missing)}), "
                               f"unexpected {unexpected[:5]} ({len(unexpected)})")
        if not missing:
            dev = self.model.positional_embedding.device
            packed = pack_state_dict(sd)
            with torch.no_grad():  # in place: captured graphs keep reading the same buffers
                for name, t in packed.items():
                    dst = self.model.positional_embedding if name == "pos" else getattr(self, name)
                    if dst.shape != t.shape:
                        raise RuntimeError(f"HipTextTower.load_state_dict: {name} {tuple(t.shape)} vs {tuple(dst.shape)}")
                    dst.copy_(t.to(dev))
        return missing, unexpected

    # ------------------------------------------------------------------ launches
    def _gemm_desc(self, M, N, K, A, lda, w, bias, out, ldo, *, act=0, stream_res=False):
        d = _lib.GemmDesc()
        d.M, d.N, d.K, d.amode = M, N, K, 0
        d.A, d.lda = A.data_ptr(), lda
        d.Wt, d.ldw = w.data_ptr(), K
        d.alpha, d.act = 1.0, act
        d.bias = bias.data_ptr()
        d.rows_per_b = 1
        d.out, d.ldo = out.data_ptr(), ldo
        if stream_res:  # x += ..., the stream's two planes read and rewritten in place
            C = self.width
            d.res, d.ld_res, d.res_lo, d.out_lo = self._xs.data_ptr(), 2 * C, C, C
        d.partial, d.partial_cap = self._part.data_ptr(), self._part.numel()
        d.tile_sem, d.sem_cap = self._sem.data_ptr(), self._sem.numel()
        bm, bn, sp, kern = (ctypes.c_int() for _ in range(4))
        _lib.check(self._L.tair_k_gemm_plan(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(sp),
                                            ctypes.byref(kern)), f"text tower GEMM plan (M {M}, N {N}, K {K}, act {act})")
        return d

    def _plan(self, B: int, L: int) -> List:
        """The launch list of a [B, L] forward: (function, arguments before the stream, name)."""
        key = (B, L)
        if key in self._plans:
            return self._plans[key]
        C, H, T, lib = self.width, self.heads, B * L, self._L
        xs, y, qkv, ao, h = self._xs, self._y, self._qkv, self._ao, self._h
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        ops = []

        def ln(g, b, dst, ldy, f32, name):
            ops.append((lib.tair_k_layernorm_split, (p(xs), 2 * C, C, T, C, p(g), p(b), LN_EPS, p(dst), ldy, f32), name))

        def gemm(d, name):
            ops.append((lib.tair_k_gemm, (ctypes.byref(d),), name))
            self._keep.append(d)

        self._keep = getattr(self, "_keep", [])
        for i in range(self.layers - self.layer_idx):
            ln(self.g_ln1[i], self.b_ln1[i], y, C, 0, "ln_1")
            gemm(self._gemm_desc(T, 3 * C, C, y, C, self.w_qkv[i], self.b_qkv[i], qkv, 3 * C), "qkv")
            ops.append((lib.tair_k_attention_causal,
                        (p(qkv), 3 * C, p(qkv[:, C:]), 3 * C, p(qkv[:, 2 * C:]), 3 * C, p(ao), C, B, H, L, 0.125), "attn"))
            gemm(self._gemm_desc(T, C, C, ao, C, self.w_out[i], self.b_out[i], xs, 2 * C, stream_res=True), "out_proj")
            ln(self.g_ln2[i], self.b_ln2[i], y, C, 0, "ln_2")
            gemm(self._gemm_desc(T, 4 * C, C, y, C, self.w_fc[i], self.b_fc[i], h, 4 * C, act=3), "c_fc")
            gemm(self._gemm_desc(T, C, 4 * C, h, 4 * C, self.w_proj[i], self.b_proj[i], xs, 2 * C, stream_res=True),
                 "c_proj")
        ln(self.g_lnf, self.b_lnf, self._out, C, 1, "ln_final")
        self._plans[key] = ops
        return ops

    def launch_count(self, B: int = 1, L: Optional[int] = None) -> int:
        """Kernel-ABI calls of one forward (a split-K GEMM that is not combined in-kernel adds a reduce launch)."""
        return 1 + len(self._plan(B, L or self.ctx))

    @torch.no_grad()
    def forward(self, tokens: torch.Tensor) -> torch.Tensor:
        dev = self.model.positional_embedding.device
        if tokens.dim() != 2 or tokens.shape[0] < 1 or tokens.shape[1] < 1 or tokens.shape[1] > self.ctx:
            raise _lib.TairError(f"HipTextTower: tokens {tuple(tokens.shape)} (batch >= 1, length 1..{self.ctx})")
        ids = tokens.to(device=dev, dtype=torch.long).contiguous()
        B, L = ids.shape
        if B > self.max_batch:  # more prompts than the workspaces hold: in runs of max_batch (never a reallocation)
            return torch.cat([self(ids[i:i + self.max_batch]) for i in range(0, B, self.max_batch)])
        C = self.width
        ops = self._plan(B, L)
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(self._L.tair_k_embed_tokens(ctypes.c_void_p(ids.data_ptr()), B, L,
                                                   ctypes.c_void_p(self.tok.data_ptr()), self.vocab,
                                                   ctypes.c_void_p(self.model.positional_embedding.data_ptr()), C,
                                                   ctypes.c_void_p(self._xs.data_ptr()), C, 2 * C, stream),
                       "text tower embed_tokens")
            for fn, args, name in ops:
                _lib.check(fn(*args, stream), f"text tower {name}")
        # (the workspace rows are contiguous per token: [B * L, C] == [B, L, C] of the first B * L rows)
        return self._out.view(-1, C)[:B * L].view(B, L, C).clone()

    @torch.no_grad()
    def encode(self, text: Union[str, List[str]]) -> torch.Tensor:
        tokens = tokenize(text, self.ctx, self._tok)
        return self(tokens.to(self.model.positional_embedding.device))

    def check_faults(self):
        """Raise when a kernel reported a fault since the last check (a token id outside the table, a
        cooperative split-K wait that timed out).  Synchronous."""
        _lib.check_faults("HipTextTower")


def build_text_tower(clip_cfg: dict, backend: str = "torch", *, device="cuda", max_batch: int = 8):
    """The text tower of ControlLDM: ``"torch"`` = the stock FrozenOpenCLIPEmbedder (the default, unchanged),
    ``"hip"`` = HipTextTower with that module's (initial) weights; anything else is an error."""
    if backend not in ("torch", "hip"):
        raise ValueError(f"clip_backend must be 'torch' or 'hip', got {backend!r}")
    if backend == "torch":
        return FrozenOpenCLIPEmbedder(**clip_cfg).to(device).eval()
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise _lib.TairError("clip_backend='hip' needs a ROCm GPU (no CPU fallback)")
    return HipTextTower(FrozenOpenCLIPEmbedder(**clip_cfg).eval(), max_batch=max_batch, device=dev).eval()
