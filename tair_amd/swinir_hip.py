"""SwinIR cleaner on the HIP kernels (reference: terediff/model/swinir.py:624-894; the stock-torch form is
tair_amd/swinir.py).  Opt-in (``config.build_swinir(..., backend="hip")``); the val-config network only.

Driven from Python over the kernel ABI (include/tair_kernels.h), as clip_hip.py drives the text tower:

* layouts are padded once so every GEMM sees K and C as multiples of 64: the 180-channel stream lives in 192
  columns (zero weight rows and zero bias for the pad, so the pad columns stay exactly zero), each of the 6 heads
  (d = 30) occupies 32 columns of q | k | v (N = 576) and of proj's K, the MLP hidden 360 is 384 (GELU(0) = 0);
  the 3x3 convs take the GEMM's channel-chunk-major K order at C = 192 / 64;
* bf16 weights and GEMM operands; the token stream is two bf16 planes hi = bf16(x), lo = bf16(x - hi) side by
  side in one [T, 2 * 192] buffer, read and rewritten in place by the residual GEMMs (proj, fc2, the group conv,
  conv_after_body) through ``res`` / ``res_lo`` / ``out_lo``.  A group's input t0 stays in one buffer (A) while its
  blocks run in a second (B): block 0's proj reads its residual from A and writes B, the group conv reads B's hi
  plane (with its 3x3 halo) and adds into A in place, so no pass copies the stream;
* the input is two planes as well: (x - mean) pixel-unshuffled to [T, 192] is split hi | lo and conv_first runs
  over C = 384 with its weights repeated for the second plane (an 8-bit image does not fit in one bf16 plane); the
  mean is subtracted before the conv, whose zero padding pads the mean-subtracted image, as in the reference;
* per block, 7 launches: norm1 (tair_k_layernorm_split_pad) -> q|k|v GEMM -> tair_k_window_attention (shift,
  window partition, relative-position bias and shift mask inside the kernel) -> proj GEMM (+ residual) -> norm2 ->
  fc1 GEMM (GELU epilogue, act 3) -> fc2 GEMM (+ residual); per group one conv GEMM; then norm, conv_after_body
  (+ conv_first's output), conv_before_upsample + LeakyReLU(0.01), three nearest-x2 upsample convs (A_CONV3_UP) +
  LeakyReLU(0.2), conv_hr + LeakyReLU(0.2), conv_last (N = 3, fp32 out, rgb_mean folded into its bias).
  2 + 7 blocks + groups + 3 + 10 launches.

The boundary conversions (mean, pixel-unshuffle, NCHW <-> NHWC, the hi / lo split of the input) are device torch
ops in ``forward``.  ``forward_tiled`` (an image larger than the workspaces: utils/common.py:174-234 as
pipeline.py:389-394 wraps the cleaner) runs the same launch list on chunks of overlapping windows between two
kernels of csrc/image_tile.hip: tair_k_image_tile_gather writes the windows as the two-plane input (the boundary
conversions inside it), tair_k_image_tile_blend adds conv_last's fp32 rows into whole-image accumulators with the
Gaussian weights in the reference loop's order and divides on the last chunk.  Workspaces are sized at construction for ``max_batch`` images of a ``max_hw`` token map; a forward launches
on the current stream only, never synchronises and is capturable.  A missing kernel or a refused plan raises
``TairError``: there is no fallback to torch.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .swinir import RGB_MEAN

LN_EPS = 1e-5
C, CP = 180, 192          # stream width, padded
HEADS, D, DP = 6, 30, 32  # heads, head dim, padded
HID, HIDP = 360, 384      # MLP hidden, padded
NF = 64                   # upsampler width
SF = 8
WS = 8
A_DENSE, A_CONV3, A_CONV3_UP = 0, 1, 3

_BLOCK_LN = {"g_ln1": "norm1.weight", "b_ln1": "norm1.bias", "g_ln2": "norm2.weight", "b_ln2": "norm2.bias"}
_TOP_LN = {"g_pn": "patch_embed.norm.weight", "b_pn": "patch_embed.norm.bias", "g_n": "norm.weight", "b_n": "norm.bias"}
# packed name -> (reference module, input channels padded to, output channels padded to)
_CONVS = {"cab": ("conv_after_body", CP, CP), "cbu": ("conv_before_upsample.0", CP, NF), "up1": ("conv_up1", NF, NF),
          "up2": ("conv_up2", NF, NF), "up3": ("conv_up3", NF, NF), "hr": ("conv_hr", NF, NF), "last": ("conv_last", NF, 3)}
# reference buffers the forward does not read (rebuilt from coordinates in the kernel)
_UNUSED_SUFFIX = ("relative_position_index", "attn_mask")


def check_params(p: dict) -> None:
    """ValueError unless p is the val-config network (config.SWINIR_VAL_PARAMS) up to its depth."""
    depths, heads = list(p.get("depths", ())), list(p.get("num_heads", ()))
    want = dict(embed_dim=C, window_size=WS, mlp_ratio=2, sf=SF, upsampler="nearest+conv", resi_connection="1conv",
                unshuffle=True, unshuffle_scale=SF, in_chans=3, patch_size=1, img_range=1.0, patch_norm=True,
                qkv_bias=True, ape=False)
    defaults = dict(in_chans=3, patch_size=1, img_range=1.0, patch_norm=True, qkv_bias=True, ape=False,
                    resi_connection="1conv", mlp_ratio=4.0, embed_dim=96, window_size=7, sf=4, upsampler="",
                    unshuffle=False, unshuffle_scale=None)
    bad = {k: p.get(k, defaults[k]) for k, v in want.items() if p.get(k, defaults[k]) != v}
    if bad or not depths or len(depths) != len(heads) or any(h != HEADS for h in heads) or any(d < 1 for d in depths):
        raise ValueError(f"HipSwinIR runs the val-config network only (embed_dim 180, 6 heads, window 8, mlp_ratio 2, "
                         f"unshuffle 8, nearest+conv x8, 1conv, patch_norm, img_range 1); got {bad or p}")


def _blk(i: int, j: int) -> str:
    return f"layers.{i}.residual_group.blocks.{j}."


def _pack_conv(w: torch.Tensor, cin_p: int, cout_p: int, planes: int = 1) -> torch.Tensor:
    """[co, ci, 3, 3] fp32 -> [cout_p, 9 * planes * cin_p] bf16 in the GEMM's channel-chunk-major K order
    k = (c / 64 * 9 + tap) * 64 + c % 64 (kernels.h A_CONV3), input channels zero-padded to cin_p and repeated
    `planes` times (a two-plane input), output rows zero-padded to cout_p."""
    co, ci = w.shape[:2]
    wt = torch.zeros((cout_p, 9, cin_p), dtype=torch.float32)
    wt[:co, :, :ci] = w.detach().float().permute(0, 2, 3, 1).reshape(co, 9, ci)
    wt = wt.repeat(1, 1, planes)
    cc = planes * cin_p
    return wt.reshape(cout_p, 9, cc // 64, 64).permute(0, 2, 1, 3).reshape(cout_p, 9 * cc).to(torch.bfloat16).contiguous()


def _unpack_conv(wp: torch.Tensor, ci: int, co: int) -> torch.Tensor:
    cc = wp.shape[1] // 9
    wt = wp.reshape(wp.shape[0], cc // 64, 9, 64).permute(0, 2, 1, 3).reshape(wp.shape[0], 9, cc)
    return wt[:co, :, :ci].reshape(co, 3, 3, ci).permute(0, 3, 1, 2).contiguous()


def _head_cols(x: torch.Tensor, dim: int, parts: int) -> torch.Tensor:
    """Regroup `dim` of length parts * 180 (head h at h * 30) into parts * 192 (head h at h * 32, zero pad)."""
    x = x.movedim(dim, -1)
    y = torch.zeros(x.shape[:-1] + (parts, HEADS, DP), dtype=x.dtype)
    y[..., :D] = x.reshape(x.shape[:-1] + (parts, HEADS, D))
    return y.reshape(x.shape[:-1] + (parts * CP,)).movedim(-1, dim)


def _unhead_cols(y: torch.Tensor, dim: int, parts: int) -> torch.Tensor:
    y = y.movedim(dim, -1)
    x = y.reshape(y.shape[:-1] + (parts, HEADS, DP))[..., :D]
    return x.reshape(y.shape[:-1] + (parts * C,)).movedim(-1, dim)


def _pad2(w: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    out = torch.zeros((rows, cols), dtype=w.dtype)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _pad1(b: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.zeros(n, dtype=b.dtype)
    out[:b.shape[0]] = b
    return out


def count_depths(sd: Dict[str, torch.Tensor]) -> List[int]:
    depths = []
    while f"layers.{len(depths)}.conv.weight" in sd:
        j = 0
        while _blk(len(depths), j) + "norm1.weight" in sd:
            j += 1
        depths.append(j)
    return depths


def pack_state_dict(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Reference-key state dict of the val-config SwinIR -> the packed tensors of HipSwinIR (on the CPU): per-block
    tensors stacked over all blocks in execution order, per-group convs over the groups; linear and conv weights
    bf16 in the padded layouts of the module docstring, everything else fp32."""
    depths = count_depths(sd)
    if not depths or min(depths) < 1:
        raise _lib.TairError("swinir_hip: no layers.*.residual_group.blocks.* keys in the state dict")
    f = lambda k: sd[k].detach().float().cpu()  # noqa: E731
    bf = torch.bfloat16
    blocks = [_blk(i, j) for i, d in enumerate(depths) for j in range(d)]
    if f("conv_first.1.weight").shape != (C, 3 * SF * SF, 3, 3) or f(blocks[0] + "attn.qkv.weight").shape != (3 * C, C) \
            or f(blocks[0] + "mlp.fc1.weight").shape != (HID, C) or \
            f(blocks[0] + "attn.relative_position_bias_table").shape != ((2 * WS - 1) ** 2, HEADS):
        raise _lib.TairError("swinir_hip: the state dict is not the val-config SwinIR's (embed_dim 180, 6 heads, "
                             "window 8, mlp_ratio 2, unshuffle 8)")
    out = {name: f(key).contiguous() for name, key in _TOP_LN.items()}
    for name, key in _BLOCK_LN.items():
        out[name] = torch.stack([f(b + key) for b in blocks]).contiguous()
    out["bias_tab"] = torch.stack([f(b + "attn.relative_position_bias_table") for b in blocks]).contiguous()
    out["w_qkv"] = torch.stack([_pad2(_head_cols(f(b + "attn.qkv.weight"), 0, 3), 3 * CP, CP) for b in blocks]).to(bf)
    out["b_qkv"] = torch.stack([_head_cols(f(b + "attn.qkv.bias"), 0, 3) for b in blocks]).contiguous()
    out["w_proj"] = torch.stack([_pad2(_head_cols(f(b + "attn.proj.weight"), 1, 1), CP, CP) for b in blocks]).to(bf)
    out["b_proj"] = torch.stack([_pad1(f(b + "attn.proj.bias"), CP) for b in blocks])
    out["w_fc1"] = torch.stack([_pad2(f(b + "mlp.fc1.weight"), HIDP, CP) for b in blocks]).to(bf)
    out["b_fc1"] = torch.stack([_pad1(f(b + "mlp.fc1.bias"), HIDP) for b in blocks])
    out["w_fc2"] = torch.stack([_pad2(f(b + "mlp.fc2.weight"), CP, HIDP) for b in blocks]).to(bf)
    out["b_fc2"] = torch.stack([_pad1(f(b + "mlp.fc2.bias"), CP) for b in blocks])
    out["w_gconv"] = torch.stack([_pack_conv(f(f"layers.{i}.conv.weight"), CP, CP) for i in range(len(depths))])
    out["b_gconv"] = torch.stack([_pad1(f(f"layers.{i}.conv.bias"), CP) for i in range(len(depths))])
    out["w_first"] = _pack_conv(f("conv_first.1.weight"), CP, CP, planes=2)
    out["b_first"] = _pad1(f("conv_first.1.bias"), CP)
    for name, (key, cin_p, cout_p) in _CONVS.items():
        out["w_" + name] = _pack_conv(f(key + ".weight"), cin_p, cout_p)
        out["b_" + name] = _pad1(f(key + ".bias"), cout_p)
    out["depths"] = torch.tensor(depths, dtype=torch.int64)
    return {k: v.contiguous() for k, v in out.items()}


def unpack_state_dict(packed: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of pack_state_dict: reference key names, the linear and conv weights as the bf16 values the
    kernels read (pads removed, heads back at 30 columns), everything else the fp32 values that were packed."""
    depths = [int(d) for d in packed["depths"]]
    out = {key: packed[name] for name, key in _TOP_LN.items()}
    n = 0
    for i, d in enumerate(depths):
        for j in range(d):
            b = _blk(i, j)
            for name, key in _BLOCK_LN.items():
                out[b + key] = packed[name][n]
            out[b + "attn.relative_position_bias_table"] = packed["bias_tab"][n]
            out[b + "attn.qkv.weight"] = _unhead_cols(packed["w_qkv"][n][:, :C], 0, 3).contiguous()
            out[b + "attn.qkv.bias"] = _unhead_cols(packed["b_qkv"][n], 0, 3).contiguous()
            out[b + "attn.proj.weight"] = _unhead_cols(packed["w_proj"][n][:C], 1, 1).contiguous()
            out[b + "attn.proj.bias"] = packed["b_proj"][n][:C]
            out[b + "mlp.fc1.weight"] = packed["w_fc1"][n][:HID, :C]
            out[b + "mlp.fc1.bias"] = packed["b_fc1"][n][:HID]
            out[b + "mlp.fc2.weight"] = packed["w_fc2"][n][:C, :HID]
            out[b + "mlp.fc2.bias"] = packed["b_fc2"][n][:C]
            n += 1
        out[f"layers.{i}.conv.weight"] = _unpack_conv(packed["w_gconv"][i], C, C)
        out[f"layers.{i}.conv.bias"] = packed["b_gconv"][i][:C]
    out["conv_first.1.weight"] = _unpack_conv(packed["w_first"], 3 * SF * SF, C)
    out["conv_first.1.bias"] = packed["b_first"][:C]
    for name, (key, _, _) in _CONVS.items():
        co = {"cab": C, "last": 3}.get(name, NF)
        ci = C if name in ("cab", "cbu") else NF
        out[key + ".weight"] = _unpack_conv(packed["w_" + name], ci, co)
        out[key + ".bias"] = packed["b_" + name][:co]
    return out


def _r64(n: int) -> int:
    return (n + 63) // 64 * 64


def gemm_desc(L, name, M, N, K, A, lda, w, bias, out, ldo, part, sem, *, act=0, res=None, res_lo=0, out_lo=0,
              out_f32=0, conv=None):
    """The planned tair_gemm_desc of one GEMM of the launch list, on raw addresses (planning reads no operand).
    part / sem: (address, capacity) of the split-K slabs and tickets; conv: (mode, channels, B, H, W, Ho, Wo);
    res: the stream's planes (res_lo = 0: one plane), read and rewritten in place when res is out.  TairError for
    a refused plan."""
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.amode = M, N, K, A_DENSE
    d.A, d.lda = A, lda
    d.Wt, d.ldw = w, K
    d.alpha, d.act = 1.0, act
    d.bias = bias
    d.rows_per_b = 1
    d.out, d.ldo, d.out_f32 = out, ldo, out_f32
    if conv is not None:
        d.amode, d.C, d.Bn, d.H, d.W, d.Ho, d.Wo = conv
        d.rows_per_b = d.Ho * d.Wo
    if res is not None:
        d.res, d.ld_res, d.res_lo = res, 2 * CP, res_lo
    d.out_lo = out_lo
    d.partial, d.partial_cap = part
    d.tile_sem, d.sem_cap = sem
    plan = [ctypes.c_int() for _ in range(4)]
    rc = L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(v) for v in plan])
    if act == 3 and (rc != 0 or abs(plan[0].value) > 128 or plan[1].value > 128):
        # the GELU epilogue is built for the <= 128 x 128 tiles: where the planner picks a wider one, force it
        d.force_bm, d.force_bn = 128, 128
        rc = L.tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(v) for v in plan])
    _lib.check(rc, f"SwinIR GEMM plan {name} (M {M}, N {N}, K {K}, act {act})")
    return d


def check_input(shape, max_hw: Tuple[int, int]) -> Tuple[int, int, int]:
    """(B, h, w) of the token maps of an input of `shape`; ValueError unless it is [B, 3, H, W] with H, W multiples
    of 64 and a token map within the max_hw the workspaces were built for."""
    if len(shape) != 4 or shape[0] < 1 or shape[1] != 3:
        raise ValueError(f"HipSwinIR: input {tuple(shape)} (need [B, 3, H, W])")
    H, W = int(shape[2]), int(shape[3])
    if H < SF * WS or W < SF * WS or H % (SF * WS) or W % (SF * WS):
        raise ValueError(f"HipSwinIR: input {H}x{W}: H and W must be multiples of {SF * WS}")
    h, w = H // SF, W // SF
    if h * w > max_hw[0] * max_hw[1]:
        raise ValueError(f"HipSwinIR: token map {h}x{w} exceeds the {max_hw[0]}x{max_hw[1]} the workspaces were "
                         "built for")
    return int(shape[0]), h, w


def check_tiled_input(shape, tile_size: int, tile_stride: int, max_hw: Tuple[int, int]) -> Tuple[int, int, int, int]:
    """(B, H, W, t) of a tiled call, t the side of a window's token map; ValueError unless the input is [B, 3, H, W]
    with H, W >= tile_size, tile_size a multiple of 64 whose token map fits max_hw, and tile_stride >= 1."""
    if len(shape) != 4 or shape[0] < 1 or shape[1] != 3:
        raise ValueError(f"HipSwinIR: input {tuple(shape)} (need [B, 3, H, W])")
    tile_size, tile_stride = int(tile_size), int(tile_stride)
    if tile_size < SF * WS or tile_size % (SF * WS):
        raise ValueError(f"HipSwinIR: tile size {tile_size} must be a multiple of {SF * WS}")
    if tile_stride < 1:
        raise ValueError(f"HipSwinIR: tile stride {tile_stride} must be >= 1")
    t = tile_size // SF
    if t * t > max_hw[0] * max_hw[1]:
        raise ValueError(f"HipSwinIR: a {tile_size} tile's token map {t}x{t} exceeds the {max_hw[0]}x{max_hw[1]} the "
                         "workspaces were built for")
    H, W = int(shape[2]), int(shape[3])
    if H < tile_size or W < tile_size:
        raise ValueError(f"HipSwinIR: image {H}x{W} is smaller than the tile {tile_size}")
    return int(shape[0]), H, W, t


class HipSwinIR(nn.Module):
    """SwinIR (val config) on the HIP kernels: ``forward(x)`` as the stock module, x [B, 3, H, W] fp32 in [0, 1]
    with H, W multiples of 64 -> [B, 3, H, W] fp32; ``forward_tiled(x, tile_size, tile_stride)`` for an image
    larger than the workspaces.  ``src``: a tair_amd.swinir.SwinIR or a reference-key state dict; ``params``: its
    constructor arguments (checked: the val-config network only)."""

    tiling = True  # SwinIRPipeline.apply_cleaner(tiled=True) is served, by forward_tiled

    def __init__(self, src, params: dict, *, max_batch: int = 4, max_hw: Tuple[int, int] = (64, 64), device="cuda"):
        super().__init__()
        check_params(params)
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise _lib.TairError("tair_amd.HipSwinIR needs a ROCm GPU (no CPU fallback)")
        sd = src.state_dict() if isinstance(src, nn.Module) else src
        packed = pack_state_dict(sd)
        if [int(d) for d in packed["depths"]] != list(params["depths"]):
            raise _lib.TairError(f"HipSwinIR: the state dict has depths {packed['depths'].tolist()}, the parameters "
                                 f"{list(params['depths'])}")
        self.max_batch = int(max_batch)
        self.max_hw = (int(max_hw[0]), int(max_hw[1]))
        if self.max_batch < 1 or min(self.max_hw) < WS or self.max_hw[0] % WS or self.max_hw[1] % WS:
            raise ValueError(f"HipSwinIR: max_batch {max_batch}, max token map {max_hw} (multiples of 8)")
        self._L = _lib.lib()
        self._plans: Dict[tuple, List] = {}
        self._keep: List = []
        self._tiled: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}  # (B, H, W, tile, stride) -> acc, cnt
        self._weights: Dict[int, torch.Tensor] = {}                      # tile -> fp32 Gaussian weights [tile, tile]
        self.last_tiling: Optional[Dict] = None                          # the plan of the last forward_tiled
        self._depths = [int(d) for d in packed["depths"]]
        for name, t in packed.items():
            self.register_buffer(name, t.to(dev).contiguous())
        self.register_buffer("mean", torch.tensor(RGB_MEAN, dtype=torch.float32, device=dev).reshape(1, 3, 1, 1),
                             persistent=False)
        self.register_buffer("b_last_mean", self.b_last + self.mean.reshape(3), persistent=False)
        T = self.max_batch * self.max_hw[0] * self.max_hw[1]
        bf = dict(dtype=torch.bfloat16, device=dev)
        # workspaces (never reallocated: a captured graph keeps pointing at them)
        self._in = torch.zeros((T, 2 * CP), **bf)   # (x - mean) unshuffled, planes hi | lo
        self._f = torch.zeros((T, 2 * CP), **bf)    # conv_first's output, then conv_after_body's
        self._xa = torch.zeros((T, 2 * CP), **bf)   # the stream at the group boundaries
        self._xb = torch.zeros((T, 2 * CP), **bf)   # the stream inside a group
        self._y = torch.zeros((T, CP), **bf)        # LayerNorm output
        self._qkv = torch.zeros((T, 3 * CP), **bf)
        self._ao = torch.zeros((T, CP), **bf)
        self._h = torch.zeros((T, HIDP), **bf)
        self._u = [torch.zeros((T * 4 ** i, NF), **bf) for i in range(4)]  # conv_before_upsample, conv_up1..3
        self._hr = torch.zeros((T * 64, NF), **bf)
        self._o32 = torch.zeros((T * 64, 3), dtype=torch.float32, device=dev)
        self._part = torch.empty(16 << 20, dtype=torch.float32, device=dev)  # split-K slabs
        self._sem = torch.zeros(1 << 16, dtype=torch.int32, device=dev)

    # ------------------------------------------------------------------ weights
    def reference_keys(self) -> set:
        return set(unpack_state_dict({k: v for k, v in self._packed().items()}))

    def _packed(self) -> Dict[str, torch.Tensor]:
        return {k: v for k, v in self.state_dict().items()}

    def load_state_dict(self, sd, strict: bool = True, **kw):
        """Reference key names (a SwinIR checkpoint's) are repacked for the kernels, in place; the module's own
        (packed) state dict loads as any module's."""
        if "conv_first.1.weight" not in sd:
            return super().load_state_dict(sd, strict=strict, **kw)
        sd = {k: v for k, v in sd.items() if not k.endswith(_UNUSED_SUFFIX)}
        want = self.reference_keys()
        missing, unexpected = sorted(want - set(sd)), sorted(set(sd) - want)
        if strict and (missing or unexpected):
            raise RuntimeError(f"HipSwinIR.load_state_dict: missing {missing[:5]} ({len(missing)}), "
                               f"unexpected {unexpected[:5]} ({len(unexpected)})")
        if not missing:
            packed = pack_state_dict(sd)
            with torch.no_grad():  # in place: captured graphs keep reading the same buffers
                for name, t in packed.items():
                    dst = getattr(self, name)
                    if dst.shape != t.shape:
                        raise RuntimeError(f"HipSwinIR.load_state_dict: {name} {tuple(t.shape)} vs {tuple(dst.shape)}")
                    dst.copy_(t.to(dst.device))
                self.b_last_mean.copy_(self.b_last + self.mean.reshape(3))
        return missing, unexpected

    # ------------------------------------------------------------------ launches
    def _desc(self, name, M, N, K, A, lda, w, bias, out, ldo, *, res=None, **kw):
        d = gemm_desc(self._L, name, M, N, K, A.data_ptr(), lda, w.data_ptr(), bias.data_ptr(), out.data_ptr(), ldo,
                      (self._part.data_ptr(), self._part.numel()), (self._sem.data_ptr(), self._sem.numel()),
                      res=None if res is None else res.data_ptr(), **kw)
        self._keep.append(d)
        return d

    def _plan(self, B: int, h: int, w: int) -> List:
        """The launch list of a forward over B token maps of h x w: (function, arguments before the stream, name)."""
        key = (B, h, w)
        if key in self._plans:
            return self._plans[key]
        T, lib = B * h * w, self._L
        xa, xb, y, qkv, ao, hid, fbuf = self._xa, self._xb, self._y, self._qkv, self._ao, self._h, self._f
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        ops = []

        def ln(src, x_lo, g, b, dst, ldy, name):
            ops.append((lib.tair_k_layernorm_split_pad, (p(src), 2 * CP, x_lo, T, C, CP, p(g), p(b), LN_EPS, p(dst), ldy),
                        name))

        def gemm(d, name):
            ops.append((lib.tair_k_gemm, (ctypes.byref(d),), name))

        def conv3(name, A, lda, cin, wt, bias, out, ldo, N, *, up=False, hh=h, ww=w, **kw):
            ho, wo = (2 * hh, 2 * ww) if up else (hh, ww)
            gemm(self._desc(name, B * ho * wo, N, 9 * cin, A, lda, wt, bias, out, ldo,
                            conv=(A_CONV3_UP if up else A_CONV3, cin, B, hh, ww, ho, wo), **kw), name)

        def leaky(buf, rows, slope, name):
            ops.append((lib.tair_k_leaky_relu, (p(buf), NF, rows, NF, slope), name))

        conv3("conv_first", self._in, 2 * CP, 2 * CP, self.w_first, self.b_first, fbuf, 2 * CP, CP, out_lo=CP)
        ln(fbuf, CP, self.g_pn, self.b_pn, xa, 2 * CP, "patch_embed.norm")  # the stream starts as one plane (lo = 0)
        a_lo, n = 0, 0
        scale = float(D) ** -0.5
        for gi, depth in enumerate(self._depths):
            for j in range(depth):
                src, s_lo = (xa, a_lo) if j == 0 else (xb, CP)
                ln(src, s_lo, self.g_ln1[n], self.b_ln1[n], y, CP, "norm1")
                gemm(self._desc("qkv", T, 3 * CP, CP, y, CP, self.w_qkv[n], self.b_qkv[n], qkv, 3 * CP), "qkv")
                ops.append((lib.tair_k_window_attention,
                            (p(qkv), 3 * CP, p(qkv[:, CP:]), 3 * CP, p(qkv[:, 2 * CP:]), 3 * CP, p(ao), CP, B, h, w, HEADS,
                             D, WS // 2 if j % 2 else 0, p(self.bias_tab[n]), scale), "window_attention"))
                gemm(self._desc("proj", T, CP, CP, ao, CP, self.w_proj[n], self.b_proj[n], xb, 2 * CP, res=src,
                                res_lo=s_lo, out_lo=CP), "proj")
                ln(xb, CP, self.g_ln2[n], self.b_ln2[n], y, CP, "norm2")
                gemm(self._desc("fc1", T, HIDP, CP, y, CP, self.w_fc1[n], self.b_fc1[n], hid, HIDP, act=3), "fc1")
                gemm(self._desc("fc2", T, CP, HIDP, hid, HIDP, self.w_fc2[n], self.b_fc2[n], xb, 2 * CP, res=xb,
                                res_lo=CP, out_lo=CP), "fc2")
                n += 1
            conv3("group conv", xb, 2 * CP, CP, self.w_gconv[gi], self.b_gconv[gi], xa, 2 * CP, CP, res=xa, res_lo=a_lo,
                  out_lo=CP)
            a_lo = CP
        ln(xa, a_lo, self.g_n, self.b_n, y, CP, "norm")
        conv3("conv_after_body", y, CP, CP, self.w_cab, self.b_cab, fbuf, 2 * CP, CP, res=fbuf, res_lo=CP, out_lo=CP)
        u = self._u
        conv3("conv_before_upsample", fbuf, 2 * CP, CP, self.w_cbu, self.b_cbu, u[0], NF, NF)
        leaky(u[0], T, 0.01, "leaky_relu 0.01")
        for i in range(3):
            conv3(f"conv_up{i + 1}", u[i], NF, NF, getattr(self, f"w_up{i + 1}"), getattr(self, f"b_up{i + 1}"), u[i + 1],
                  NF, NF, up=True, hh=h << i, ww=w << i)
            leaky(u[i + 1], T * 4 ** (i + 1), 0.2, "leaky_relu 0.2")
        conv3("conv_hr", u[3], NF, NF, self.w_hr, self.b_hr, self._hr, NF, NF, hh=8 * h, ww=8 * w)
        leaky(self._hr, 64 * T, 0.2, "leaky_relu 0.2")
        conv3("conv_last", self._hr, NF, NF, self.w_last, self.b_last_mean, self._o32, 3, 3, hh=8 * h, ww=8 * w, out_f32=1)
        self._plans[key] = ops
        return ops

    def launch_count(self, B: int = 1, hw: Optional[Tuple[int, int]] = None) -> int:
        """Kernel-ABI calls of one forward (a split-K GEMM that is not combined in-kernel adds a reduce launch)."""
        h, w = hw or self.max_hw
        return len(self._plan(B, h, w))

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> torch.Tensor:
        B, h, w = check_input(x.shape, self.max_hw)
        dev = self.mean.device
        if B > self.max_batch:  # more images than the workspaces hold: in runs of max_batch (never a reallocation)
            return torch.cat([self(x[i:i + self.max_batch]) for i in range(0, B, self.max_batch)])
        T = B * h * w
        ops = self._plan(B, h, w)
        u = F.pixel_unshuffle(x.to(device=dev, dtype=torch.float32) - self.mean, SF).permute(0, 2, 3, 1).reshape(T, CP)
        hi = u.to(torch.bfloat16)
        self._in[:T, :CP].copy_(hi)
        self._in[:T, CP:].copy_(u - hi.float())
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for fn, args, name in ops:
                _lib.check(fn(*args, stream), f"SwinIR {name}")
        return self._o32[:64 * T].view(B, SF * h, SF * w, 3).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def forward_tiled(self, x: torch.Tensor, tile_size: int, tile_stride: int) -> torch.Tensor:
        """The cleaner over an image larger than the workspaces (utils/common.py:174-234 make_tiled_fn as
        pipeline.py:389-394 wraps the cleaner): x [B, 3, H, W] fp32 with H, W >= tile_size (any size: no padding, a
        window may start at any pixel), tile_size a multiple of 64 whose token map fits max_hw -> [B, 3, H, W] fp32.
        The B x T window rows run in equal chunks of at most max_batch (tiling.plan_image_tiles); per chunk
        tair_k_image_tile_gather writes the windows as the network's input, the launch list of forward runs on them
        unchanged, and tair_k_image_tile_blend adds conv_last's output into whole-image fp32 accumulators in the
        reference loop's order, dividing by the accumulated weight on the last chunk.  The accumulators and weights
        are kept per (B, H, W, tile, stride) and the first chunk starts them from zero, so the call holds no state:
        it launches on the current stream only, never synchronises and is capturable as a whole.  ``last_tiling``
        holds the plan of the last call."""
        from .tiling import gaussian_weights, plan_image_tiles
        B, H, W, t = check_tiled_input(x.shape, tile_size, tile_stride, self.max_hw)
        tile_size, tile_stride = int(tile_size), int(tile_stride)
        plan = plan_image_tiles(B, H, W, tile_size, tile_stride, self.max_batch)
        dev = self.mean.device
        rpc = plan["rows_per_chunk"]
        ops = self._plan(rpc, t, t)
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        if tile_size not in self._weights:
            self._weights[tile_size] = torch.tensor(gaussian_weights(tile_size, tile_size), dtype=torch.float32).to(dev)
        key = (B, H, W, tile_size, tile_stride)
        if key not in self._tiled:
            self._tiled[key] = (torch.empty((B, 3, H, W), dtype=torch.float32, device=dev),
                                torch.empty((B, 3, H, W), dtype=torch.float32, device=dev))
        acc, cnt = self._tiled[key]
        wts = self._weights[tile_size]
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
        lib = self._L
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for c, (first, _) in enumerate(plan["chunks"]):
                _lib.check(lib.tair_k_image_tile_gather(p(x), p(self.mean), B, H, W, tile_size, tile_stride, first, rpc,
                                                        p(self._in), 2 * CP, CP, stream), "SwinIR image_tile_gather")
                for fn, args, name in ops:
                    _lib.check(fn(*args, stream), f"SwinIR {name}")
                _lib.check(lib.tair_k_image_tile_blend(p(self._o32), p(wts), p(acc), p(cnt), p(out), B, H, W, tile_size,
                                                       tile_stride, first, rpc, int(c == plan["n_chunks"] - 1), stream),
                           "SwinIR image_tile_blend")
        self.last_tiling = plan
        return out

    def check_faults(self):
        """Raise when a kernel reported a fault since the last check (a cooperative split-K wait that timed
        out).  Synchronous."""
        _lib.check_faults("HipSwinIR")
