"""Exact-answer cases for the bf16 / fp8 MFMA GEMM and implicit-GEMM conv families (tair_k_gemm) and the d = 64 flash
attention (tair_k_attention*): operands, integer references and the case tables shared by tests/test_exact_cases_cpu.py
(no device: the exactness and coverage conditions on the operands, and every case resolves to the plan it names) and
by tests/test_gemm_exact_gpu.py / tests/test_attention_exact_gpu.py (every case, bit for bit, on the device).

GEMM and conv.  With small-integer operands every product, every partial sum and every split-K slab is an integer that
fp32 holds exactly, so the summation order, the K split, the ring depth and the tile shape cannot change a bit and the
output has one right answer, which an int64 reference gives.  The operand rule:

* activations are -1 / 0 / +1 with a fixed number of non-zeros per pixel (A_NNZ of the C channels, A_NNZ_DENSE of a
  dense row, X_NNZ of a K-extension row), so that sum_k |a| |w| <= 9 * 22 + 2 * 16 = 230 whatever the weights are;
* weights are -1 / 0 / +1.  Output row n of a 64-column block of r rows holds the K positions k = n (mod r) -- the
  block's rows together cover every tap of every channel and every K-extension column, so a K element dropped anywhere
  changes some output by at least 1 -- and random others up to W_NNZ: at most max(W_NNZ, ceil(Ktot / r)) non-zeros;
* bias, time-embedding rows and the residual are integers of magnitude <= 8;
* alpha is 1, or 0.5 with scale_bias (bias and residual only: |v| <= 0.5 (230 + 8) + 8 = 127, a half-integer that
  bf16 holds exactly below 128).
Hence sum_k |a||w| + |bias| + |emb| + |res| <= 254 <= 256: the answer is an integer (or half-integer) of at most 8
significant bits, exact in bf16, in fp32 and in the hi plane of a hi / lo pair (whose lo plane is then zero).

Every GPU input lives in a buffer with NaN guard rows above and below and NaN padding columns (lda, ldx, ld_res,
ld_emb larger than the width, ldw larger than K + Kx; e4m3 buffers carry the NaN byte 0x7f); a conv input has at
least W + 2 guard rows, so that a padding tap which is loaded and multiplied by zero instead of selected away reads NaN.

A case names its operand source, its epilogue feature set, the forced plan (force_bm, force_bn, force_splits,
force_stages) or None for the planner's own, the split-K combine, and the (kernel, bm, bn, splits) that gemm_grouped
(tair_amd/csrc/gemm.hip) resolves the request to.  For a forced plan that is expect_forced() below, written from the
launcher's rules: the kernel follows force_stages; the 4-phase kernel never splits; a split count is lowered until no K
slice is empty (slices of ceil(units / splits) K-tiles, units = K-tiles of 64, of 32 on the BK = 32 rings, 64-channel
chunks on the halo tiles).  The planner's own plans are derived by hand at the case.

Attention.  Per (batch, head) a target set T of at most 64 keys: key t in T is a distinct row of the 64 x 64 Hadamard
matrix, every other key is zero, query i is 32 x the Hadamard row of its target.  With scale 0.125 the target's score
is 256 and every other 0, so the other weights are e^-256 = 0 in fp32 and the output row is V[t(i)], bit for bit, under
every plan: a split without the target carries merge weight 2^(0 - 369) l = 0, the target's split weight 1.
"""
import ctypes
import zlib
from typing import Dict, List, Optional, Tuple

import torch

A_DENSE, A_CONV3, A_CONV3_S2, A_CONV3_UP, A_SMALLC = 0, 1, 2, 3, 4
K_TILE, K_PHASE, K_SHALLOW, K_HALO, K_DEEP, K_KGROUP = 0, 1, 2, 3, 4, 5
A_NNZ, A_NNZ_DENSE, X_NNZ, W_NNZ, SMALL = 22, 198, 16, 48, 8
F8_A_NNZ, F8_A_NNZ_DENSE, F8_X_NNZ = 6, 60, 4  # fp8: 9 * 6 + 2 * 4 = 62, times a scale of at most 4, + 8 <= 256
E4M3_ONE, E4M3_NAN = 0x38, 0x7F
T3 = 3  # force_stages of the 3-stage tile kernels

TILES = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (128, 320), (256, 128), (256, 160), (256, 256),
         (256, 320)]
RINGS = [(64, 64), (64, 128), (128, 128), (128, 256), (128, 320), (256, 128), (256, 256)]
PHASES = [(256, 256), (256, 320)]
SHALLOWS = [(64, 64), (64, 128)]
DEEPS = [(64, s) for s in (4, 5, 6, 8)] + [(128, s) for s in (4, 5, 6)]  # (bn, ring depth)
KGROUPS = [(64, 64), (64, 128)]
F8_TILES = [(64, 64), (64, 128), (128, 128), (128, 256), (128, 320)]
HALO_BN = {16: (128, 160, 192), 32: (128, 160, 192), 64: (64, 128, 160)}

# epilogue feature sets (a bias always, except on fp8 operands: see Ops)
EPI = {
    "b": dict(),
    "be": dict(emb=True),
    "br": dict(res=True),
    "ber": dict(emb=True, res=True),
    "lo": dict(out_lo=True, res=True),
    "f32": dict(out_f32=True, emb=True),
    "sp1": dict(out_split=1),
    "sp2": dict(out_split=2, res=True),
    "half": dict(half=True, res=True),
    "half32": dict(half=True, out_f32=True),
}


def cdiv(a, b):
    return (a + b - 1) // b


# ---- operand sources ------------------------------------------------------------------------------------------
def dense(M, K, Kx=0, x_wrap=0, f8=0):
    return ("dense", A_DENSE, M, K, Kx, x_wrap, f8)


def conv(amode, B, H, W, C, Kx=0, x_wrap=0, f8=0, s2_shift=0):
    return ("conv", amode, B, H, W, C, Kx, x_wrap, f8, s2_shift)


def out_hw(src) -> Tuple[int, int]:
    _, amode, _, H, W = src[:5]
    return (H // 2, W // 2) if amode == A_CONV3_S2 else (2 * H, 2 * W) if amode == A_CONV3_UP else (H, W)


def src_shape(src) -> Tuple[int, int, int]:
    """(batch elements, rows per batch element, M) of a source's output."""
    if src[0] == "dense":
        M = src[2]
        rpb = cdiv(M, 3)
        return cdiv(M, rpb), rpb, M
    Ho, Wo = out_hw(src)
    return src[2], Ho * Wo, src[2] * Ho * Wo


def src_k(src) -> Tuple[int, int, int]:
    """(K of the descriptor in bf16 elements -- byte pairs for fp8 --, real reduction length, Kx)."""
    if src[0] == "dense":
        _, _, _, K, Kx, _, f8 = src
        return (K // 2 if f8 else K), K, Kx
    _, amode, _, _, _, C, Kx, _, f8, _ = src
    if f8:
        return cdiv(9 * C, 128) * 128 // 2, 9 * C, Kx
    return cdiv(9 * C, 64) * 64, 9 * C, Kx


class Case:
    def __init__(self, name, src, N, epi, force, expect, combine=None, refusal=None, lane=0):
        self.name, self.src, self.N, self.epi, self.force = name, src, N, epi, force
        self.expect = tuple(expect) if expect is not None else None
        self.combine, self.refusal = combine, refusal
        self.lane = lane  # the operand set's lane salt (a GroupCase's second lane: 1)

    @property
    def is_conv(self):
        return self.src[0] == "conv"

    def __repr__(self):
        return self.name


def k_units(src, force) -> int:
    """K units a split count is clamped to: 64-channel chunks (halo), K-tiles of 32 (rings) or of 64 (128 fp8 values)."""
    Kd, _, Kx = src_k(src)
    if force[3] == 9:
        return src[5] // 64
    return (Kd + Kx) // (32 if force[0] < 0 else 64)


def expect_forced(src, force) -> Tuple[int, int, int, int]:
    bm, bn, splits, stages = force
    kern = K_KGROUP if stages >= 200 else K_DEEP if stages >= 100 else K_HALO if stages == 9 else \
        K_PHASE if stages >= 4 else K_SHALLOW if stages == 2 else K_TILE
    if kern == K_PHASE:
        splits = 1
    units = k_units(src, force)
    while splits > 1 and (splits - 1) * cdiv(units, splits) >= units:
        splits -= 1
    return kern, bm, bn, splits


CASES: List[Case] = []
REFUSALS: List[Case] = []


def _add(name, src, N, epi, force, combine=None, expect=None):
    if expect is None:
        expect = expect_forced(src, force)
    if expect[3] == 1:
        combine = None
    CASES.append(Case(name, src, N, epi, force, expect, combine))


def _fname(kind, bm, bn, extra=""):
    return f"{kind}{abs(bm)}x{bn}{extra}"


# ---- dense ----------------------------------------------------------------------------------------------------
D_M = (1, 63, 65, 130, 257)
D_N = (4, 70, 129, 200, 321)
D_K = (64, 192, 320)
D_K_RING = (64, 96, 160, 192, 320)
D_EPI = ("b", "br", "be", "lo", "f32", "sp1", "half", "ber", "sp2", "half32")


def _dense_family(kind, plans, ks, fam0):
    """Five cases per plan: the diagonal (M[i], N[i + f], K[i + f]) of the shape grid, f the plan's number, so that the
    plans of a family together meet every M with every N, and every plan every M, N and K value; the K-extension and
    the feature sets rotate along."""
    for f, (bm, bn, stages, tag) in enumerate(plans):
        for i, M in enumerate(D_M):
            g = fam0 + f
            N, K = D_N[(i + g) % 5], ks[(i + g) % len(ks)]
            Kx = (0, 64, 0, 128)[(i + g) % 4]
            xw = 64 if Kx == 128 else 0
            epi = D_EPI[(3 * i + g) % len(D_EPI)]
            _add(f"{_fname(kind, bm, bn, tag)}-dense-m{M}n{N}k{K}" + (f"x{Kx}" if Kx else "") + f"-{epi}",
                 dense(M, K, Kx, xw), N, epi, (bm, bn, 1, stages))


_dense_family("tile", [(bm, bn, T3, "") for bm, bn in TILES], D_K, 0)
_dense_family("ring", [(-bm, bn, 0, "") for bm, bn in RINGS], D_K_RING, 1)
_dense_family("phase", [(bm, bn, 4, "") for bm, bn in PHASES], D_K, 2)
_dense_family("shallow", [(bm, bn, 2, "") for bm, bn in SHALLOWS], D_K, 3)
_dense_family("deep", [(64, bn, 100 + s, f"s{s}") for bn, s in DEEPS], D_K, 4)
_dense_family("kgroup", [(bm, bn, 203, "") for bm, bn in KGROUPS], D_K, 0)
# the deep ring deeper than the K loop (one K-tile) at every depth, and the two-K-group tiles at odd and even K-tile
# counts (1 .. 6) -- the diagonals above reach only some of these
for _bn, _s in DEEPS:
    _add(f"deep64x{_bn}s{_s}-dense-m130n200k64-br", dense(130, 64), 200, "br", (64, _bn, 1, 100 + _s))
for _bm, _bn in KGROUPS:
    for _kt in (1, 2, 3, 4, 5, 6):
        _add(f"kgroup64x{_bn}-dense-m65n129k{64 * _kt}-b", dense(65, 64 * _kt), 129, "b", (64, _bn, 1, 203))

# ---- split-K, dense: K = 320 (five K-tiles of 64, ten of 32) in 2 slices (3 + 2 K-tiles), 5 (one each) and 7 (more
# than there are: the launcher lowers it to 5); on the rings 3 of 10 (4 + 4 + 2), 10 and 12 -> 10
SPLIT_SRC = dense(130, 320)
SPLIT_SRC_X = dense(257, 256, 64)


def _split_family(kind, bm, bn, stages, counts, modes, tag=""):
    for s in counts:
        for mode in modes:
            src, N, epi = (SPLIT_SRC, 200, "br") if s != counts[0] else (SPLIT_SRC_X, 321 if bn > 128 else 70, "lo")
            _add(f"{_fname(kind, bm, bn, tag)}-dense-s{s}-{mode}", src, N, epi, (bm, bn, s, stages), mode)


for _bm, _bn in TILES:
    _split_family("tile", _bm, _bn, T3, (2, 5, 7), ("coop", "last", "reduce") if _bm == 64 else ("reduce",))
for _bm, _bn in RINGS:
    _split_family("ring", -_bm, _bn, 0, (3, 10, 12), ("reduce",))
for _bn, _s in DEEPS:
    _split_family("deep", 64, _bn, 100 + _s, (2, 5, 7), ("last", "reduce"), f"s{_s}")
for _bm, _bn in KGROUPS:
    _split_family("kgroup", _bm, _bn, 203, (2, 5, 7), ("coop", "last", "reduce"))

# ---- stride-1 conv --------------------------------------------------------------------------------------------
C_SHAPES = ((1, 8, 8), (2, 8, 16), (2, 16, 8), (3, 5, 7), (1, 1, 1), (1, 30, 24))
C_C = (64, 128, 192)
C_N = (4, 64, 72, 200)
C_EPI = ("b", "be", "br", "ber", "lo", "f32", "half", "sp1")
C_KX = ((0, 0), (64, 0), (128, 64), (0, 0))  # (Kx, x_wrap)


def _conv_family(kind, plans, fam0):
    """Six cases per plan, one per image shape, with C, Cout, the K-extension (none / 64 / x_wrap) and the feature
    sets (time embedding, residual, both, neither, ...) rotating so that a family meets every value of each."""
    for f, (bm, bn, stages, tag) in enumerate(plans):
        for i, (B, H, W) in enumerate(C_SHAPES):
            g = fam0 + f
            C, N = C_C[(i + g) % 3], C_N[(i + g) % 4]
            Kx, xw = C_KX[(i + 2 * g + 1) % 4]
            epi = C_EPI[(i + 3 * g) % len(C_EPI)]
            _add(f"{_fname(kind, bm, bn, tag)}-conv{B}x{H}x{W}c{C}n{N}" + (f"x{Kx}" if Kx else "") +
                 ("w" if xw else "") + f"-{epi}", conv(A_CONV3, B, H, W, C, Kx, xw), N, epi, (bm, bn, 1, stages))


_conv_family("tile", [(bm, bn, T3, "") for bm, bn in TILES], 0)
_conv_family("ring", [(-bm, bn, 0, "") for bm, bn in RINGS], 1)
_conv_family("phase", [(bm, bn, 4, "") for bm, bn in PHASES], 2)
_conv_family("deep", [(64, bn, 100 + s, f"s{s}") for bn, s in DEEPS], 3)
_conv_family("kgroup", [(bm, bn, 203, "") for bm, bn in KGROUPS], 0)
# split-K convs: C = 64 + a K-extension of 64 (ten K-tiles: 3 -> 4 + 4 + 2, 10, 12 -> 10) on images whose row tiles
# straddle image boundaries
CS_SRC = conv(A_CONV3, 3, 5, 7, 64, 64)
for _kind, _bm, _bn, _st, _modes in (("tile", 64, 64, T3, ("coop", "last", "reduce")),
                                     ("tile", 64, 128, T3, ("coop", "last", "reduce")),
                                     ("tile", 128, 128, T3, ("reduce",)), ("tile", 256, 160, T3, ("reduce",)),
                                     ("ring", -64, 128, 0, ("reduce",)), ("ring", -128, 256, 0, ("reduce",)),
                                     ("deep", 64, 64, 104, ("last", "reduce")), ("deep", 64, 128, 106, ("last", "reduce")),
                                     ("kgroup", 64, 64, 203, ("coop", "last", "reduce")),
                                     ("kgroup", 64, 128, 203, ("coop", "last", "reduce"))):
    for _s in (3, 10, 12):
        for _mode in _modes:
            _add(f"{_fname(_kind, _bm, _bn)}{'s' + str(_st - 100) if _st > 100 and _st < 200 else ''}-conv3x5x7c64n72x64"
                 f"-s{_s}-{_mode}", CS_SRC, 72, "ber", (_bm, _bn, _s, _st), _mode)

# ---- halo tiles -----------------------------------------------------------------------------------------------
H_SHAPES = ((1, 16, 16), (1, 8, 32), (2, 32, 16), (1, 24, 32), (1, 4, 64), (1, 64, 64))
H_EPI = ("b", "be", "br", "ber", "lo", "f32")
for _i, (_B, _H, _W) in enumerate(H_SHAPES):
    for _j, _bn in enumerate(HALO_BN[_W]):
        for _q, _s in enumerate((1, 2, 3)):  # 3 = C / 64
            _N = (64, 72, 200)[(_i + _j + _q) % 3]
            _epi = H_EPI[(_i + 2 * _j + _q) % len(H_EPI)]
            _add(f"halo256x{_bn}-conv{_B}x{_H}x{_W}c192n{_N}-s{_s}-{_epi}", conv(A_CONV3, _B, _H, _W, 192), _N, _epi,
                 (256, _bn, _s, 9), "reduce")
    # one and two 64-channel chunks: a split count above the chunk count is lowered to it
    _add(f"halo256x{HALO_BN[_W][0]}-conv{_B}x{_H}x{_W}c64n64-s2-b", conv(A_CONV3, _B, _H, _W, 64), 64, "b",
         (256, HALO_BN[_W][0], 2, 9), "reduce")
    _add(f"halo256x{HALO_BN[_W][1]}-conv{_B}x{_H}x{_W}c128n200-s2-br", conv(A_CONV3, _B, _H, _W, 128), 200, "br",
         (256, HALO_BN[_W][1], 2, 9), "reduce")

# ---- stride 2, fused nearest-2x upsample, small-channel mode ---------------------------------------------------------
S2_SHAPES = ((1, 8, 8), (2, 8, 16), (2, 16, 8), (1, 2, 2))
S2_PLANS = ((64, 64, 1, T3), (128, 128, 1, T3), (128, 256, 1, T3), (-64, 64, 1, 0), (256, 256, 1, 4), (64, 128, 2, T3))
for _i, (_B, _H, _W) in enumerate(S2_SHAPES):
    for _sh in (0, 1):
        for _f, _force in enumerate(S2_PLANS):
            _C, _N = C_C[(_i + _f) % 2], (64, 72, 4, 200)[(_i + _f + _sh) % 4]
            _epi = C_EPI[(_i + _f + 3 * _sh) % len(C_EPI)]
            _kind = "phase" if _force[3] == 4 else "ring" if _force[0] < 0 else "tile"
            _add(f"{_fname(_kind, _force[0], _force[1])}-s2conv{_B}x{_H}x{_W}c{_C}n{_N}-shift{_sh}-s{_force[2]}-{_epi}",
                 conv(A_CONV3_S2, _B, _H, _W, _C, 0, 0, 0, _sh), _N, _epi, _force, "reduce")
UP_SHAPES = ((1, 4, 4), (2, 4, 8), (2, 8, 4), (1, 1, 1))
UP_PLANS = ((64, 64, 1, T3), (128, 128, 1, T3), (256, 128, 1, T3), (-128, 128, 1, 0), (256, 320, 1, 4), (64, 128, 3, T3))
for _i, (_B, _H, _W) in enumerate(UP_SHAPES):
    for _f, _force in enumerate(UP_PLANS):
        _C, _N = C_C[(_i + _f) % 3], (64, 72, 4, 200)[(_i + _f) % 4]
        _epi = C_EPI[(_i + 2 * _f) % len(C_EPI)]
        _kind = "phase" if _force[3] == 4 else "ring" if _force[0] < 0 else "tile"
        _add(f"{_fname(_kind, _force[0], _force[1])}-upconv{_B}x{_H}x{_W}c{_C}n{_N}-s{_force[2]}-{_epi}",
             conv(A_CONV3_UP, _B, _H, _W, _C), _N, _epi, _force, "coop")
for _i, (_B, _H, _W) in enumerate(((1, 8, 8), (2, 8, 16), (3, 5, 7))):
    for _C in (4, 8):
        for _j, _bn in enumerate((64, 128)):
            _N = (64, 72)[(_i + _j) % 2]
            _epi = ("b", "be", "br", "lo", "f32", "half")[(2 * _i + _j + _C // 8) % 6]
            _add(f"reg64x{_bn}-smallc{_B}x{_H}x{_W}c{_C}n{_N}-{_epi}", conv(A_SMALLC, _B, _H, _W, _C), _N, _epi,
                 (64, _bn, 1, T3))
_add("reg64x64-smallc2x8x16c8n72-s2-br", conv(A_SMALLC, 2, 8, 16, 8), 72, "br", (64, 64, 2, T3), "reduce")

# ---- fp8 (e4m3 operands, power-of-two row / column scales, the bf16 K-extension after the fp8 K-tiles) --------------
F8_EPI = ("b", "br", "f32", "lo")
for _f, (_bm, _bn) in enumerate(F8_TILES):
    for _i, (_M, _N, _K) in enumerate(((65, 70, 128), (257, 200, 384), (65, 200, 256), (257, 70, 640))):
        _s = (1, 2, 1, 3)[(_i + _f) % 4]
        _add(f"f8tile{_bm}x{_bn}-dense-m{_M}n{_N}k{_K}-s{_s}-{F8_EPI[(_i + _f) % 4]}", dense(_M, _K, 0, 0, 1), _N,
             F8_EPI[(_i + _f) % 4], (_bm, _bn, _s, 0), "last" if _bm == 64 else "reduce")
    for _i, (_B, _H, _W) in enumerate(((2, 8, 16), (3, 5, 7))):
        for _j, _C in enumerate((64, 128)):
            _Kx, _xw = C_KX[(_i + _j + _f) % 4]
            _N = (70, 200)[(_i + _j) % 2]
            _s = (1, 2)[(_i + _f) % 2]
            _add(f"f8tile{_bm}x{_bn}-conv{_B}x{_H}x{_W}c{_C}n{_N}" + (f"x{_Kx}" if _Kx else "") + ("w" if _xw else "") +
                 f"-s{_s}-{F8_EPI[(_i + _j + _f) % 4]}", conv(A_CONV3, _B, _H, _W, _C, _Kx, _xw, 1), _N,
                 F8_EPI[(_i + _j + _f) % 4], (_bm, _bn, _s, 0), "reduce")

# ---- the planner's own plans (gemm_plan + gemm_grouped, by hand) ----------------------------------------------------
# conv 1 x 30 x 24, C = 64 -> N = 64: M = 720 < 2048, BNc = 64 (N < 256): 12 tiles, split toward 400 workgroups with
#   >= 3 K-tiles per slice: min(33, 9 / 3) = 3; one image, but 12 < 32 tiles: no two-K-group plan
_add("own-conv1x30x24c64n64-be", conv(A_CONV3, 1, 30, 24, 64), 64, "be", None, "coop", (K_TILE, 64, 64, 3))
# dense 257 x 200 x 320: short K, M < 16384: 64 x 64 tiles, 5 x 4 = 20 tiles, (200 + 10) / 20 = 10 slices capped at
#   2 * 5 / 5 = 2
_add("own-dense-m257n200k320-br", dense(257, 320), 200, "br", None, "coop", (K_TILE, 64, 64, 2))
# dense with a K-extension (the composite FF-out rule, one lane): 5 x 4 = 20 tiles of 64 x 64, no slice count c with
#   ktiles / c >= 10 at 6 K-tiles: unsplit
_add("own-dense-m257n200k320x64-lo", dense(257, 320, 64), 200, "lo", None, "coop", (K_TILE, 64, 64, 1))
# stride-2 conv 2 x 16 x 8 -> 2 x 8 x 4, C = 128 -> N = 200: narrow (N <= 640): 64-column tiles, 1 x 4 tiles, target
#   480 -> min(120, 18 / 3, 6) = 6 slices of 3 K-tiles
_add("own-s2conv2x16x8c128n200-b", conv(A_CONV3_S2, 2, 16, 8, 128), 200, "b", None, "coop", (K_TILE, 64, 64, 6))
# fp8 dense 257 x 200 x 640 values (5 K-tiles of 128): M < 4096: 64 x 64 tiles, 20 tiles, (240 + 10) / 20 = 12
#   capped at 5 / 2 = 2
_add("own-f8-dense-m257n200k640-b", dense(257, 640, 0, 0, 1), 200, "b", None, "last", (K_TILE, 64, 64, 2))

CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES), [c.name for c in CASES if sum(d.name == c.name for d in CASES) > 1]

# ---- forced plans the library must refuse (tests/test_exact_cases_cpu.py; none of them reaches the GPU) --------------
for _name, _src, _N, _force, _msg in (
        ("refuse-shallow-split", dense(130, 320), 200, (64, 64, 2, 2), "2-stage tiles"),
        ("refuse-shallow-128x128", dense(130, 320), 200, (128, 128, 1, 2), "2-stage tiles"),
        ("refuse-shallow-conv", conv(A_CONV3, 1, 8, 8, 64), 64, (64, 64, 1, 2), "2-stage tiles"),
        ("refuse-deep-s7", dense(130, 320), 200, (64, 64, 1, 107), "deep-ring tile"),
        ("refuse-deep-128s8", dense(130, 320), 200, (64, 128, 1, 108), "deep-ring tile"),
        ("refuse-deep-s2conv", conv(A_CONV3_S2, 1, 8, 8, 64), 64, (64, 64, 1, 104), "deep-ring tile"),
        ("refuse-kgroup-128x128", dense(130, 320), 200, (128, 128, 1, 203), "two-K-group tile"),
        ("refuse-kgroup-upconv", conv(A_CONV3_UP, 1, 4, 4, 64), 64, (64, 64, 1, 203), "two-K-group tile"),
        ("refuse-halo-w24", conv(A_CONV3, 1, 30, 24, 64), 64, (256, 128, 1, 9), "halo tiles"),
        ("refuse-halo-w8", conv(A_CONV3, 1, 8, 8, 64), 64, (256, 128, 1, 9), "halo tiles"),
        ("refuse-halo-kext", conv(A_CONV3, 1, 16, 16, 64, 64), 64, (256, 128, 1, 9), "halo tiles"),
        ("refuse-halo-bn64-w16", conv(A_CONV3, 1, 16, 16, 64), 64, (256, 64, 1, 9), "halo tiles"),
        ("refuse-17-splits", dense(130, 320), 200, (64, 64, 17, T3), "K splits"),
        ("refuse-tile-k96", dense(130, 96), 200, (64, 64, 1, T3), "not a multiple of 64"),
        ("refuse-tile-64x256", dense(130, 320), 200, (64, 256, 1, T3), "not built"),
        ("refuse-ring-64x256", dense(130, 320), 200, (-64, 256, 1, 0), "not built"),
        ("refuse-phase-128x256", dense(130, 320), 200, (128, 256, 1, 4), "4-phase kernel"),
        ("refuse-smallc-128x128", conv(A_SMALLC, 1, 8, 8, 4), 64, (128, 128, 1, T3), "not built"),
        ("refuse-f8-ring", dense(65, 128, 0, 0, 1), 70, (-64, 64, 1, 0), "fp8 operands"),
        ("refuse-f8-256x128", dense(65, 128, 0, 0, 1), 70, (256, 128, 1, 0), "fp8 tile"),
        ("refuse-f8-s2conv", conv(A_CONV3_S2, 1, 8, 8, 64, 0, 0, 1), 64, (64, 64, 1, 0), "fp8 operands")):
    REFUSALS.append(Case(_name, _src, _N, "b", _force, None, None, _msg))


# ---- operands and the integer reference ----------------------------------------------------------------------------
def _signs(shape, gen):
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).to(torch.int8)


def _sparse_rows(rows, width, nnz, gen):
    """[rows, width] int8 of -1 / 0 / +1 with exactly min(nnz, width) non-zeros per row."""
    nnz = min(nnz, width)
    pos = torch.rand(rows, width, generator=gen).argsort(1)[:, :nnz]
    out = torch.zeros(rows, width, dtype=torch.int8)
    out.scatter_(1, pos, _signs((rows, nnz), gen))
    return out


def weight_cap(N, ktot, n) -> int:
    """The cap on the non-zeros of output row n: max(W_NNZ, ceil(ktot / rows of n's 64-column block))."""
    r = min(64, N - n // 64 * 64)
    return max(W_NNZ, cdiv(ktot, r))


def _weights(N, ktot, gen):
    """[N, ktot] int8: row n of a 64-column block of r rows holds every position k = n (mod r), and random others up
    to W_NNZ non-zeros."""
    w = torch.zeros(N, ktot, dtype=torch.int8)
    extra = _sparse_rows(N, ktot, W_NNZ, gen)
    sg = _signs((N, ktot), gen)
    for n0 in range(0, N, 64):
        r = min(64, N - n0)
        for j in range(r):
            cover = torch.zeros(ktot, dtype=torch.bool)
            cover[j::r] = True
            row = torch.where(cover, sg[n0 + j], torch.zeros_like(sg[n0 + j]))
            need = W_NNZ - int(cover.sum())
            if need > 0:
                cand = ((extra[n0 + j] != 0) & ~cover).nonzero().flatten()[:need]
                row[cand] = extra[n0 + j][cand]
            w[n0 + j] = row
    return w


def im2col(a: torch.Tensor, amode: int, s2_shift: int = 0) -> torch.Tensor:
    """[B, H, W, C] -> [B Ho Wo, 9, C]: tap (ky, kx) of output pixel (yo, xo), zero outside the image.  Stride 1 and the
    small-channel mode read input (yo + ky - 1, xo + kx - 1); stride 2 reads (2 yo + ky - 1 + s2_shift, ...); the
    fused upsample reads the nearest-2x upsampled image, input ((yo + ky - 1) >> 1, ...)."""
    B, H, W, C = a.shape
    if amode == A_CONV3_UP:
        a = a.repeat_interleave(2, 1).repeat_interleave(2, 2)
        H, W = 2 * H, 2 * W
    s = 2 if amode == A_CONV3_S2 else 1
    Ho, Wo = H // s, W // s
    off = s2_shift if amode == A_CONV3_S2 else 0
    p = torch.zeros(B, H + 3, W + 3, C, dtype=a.dtype, device=a.device)  # row / column 0: the -1 border
    p[:, 1:H + 1, 1:W + 1] = a
    cols = [p[:, ky + off:ky + off + s * Ho:s, kx + off:kx + off + s * Wo:s] for ky in range(3) for kx in range(3)]
    return torch.stack(cols, 3).reshape(B * Ho * Wo, 9, C)


def int_matmul(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """a [M, K] @ w [N, K]^T in int64, one output column at a time over w's non-zeros (no integer BLAS needed)."""
    a = a.to(torch.int64)
    out = torch.zeros(a.shape[0], w.shape[0], dtype=torch.int64, device=a.device)
    for n in range(w.shape[0]):
        idx = w[n].nonzero().flatten()
        if idx.numel():
            out[:, n] = (a[:, idx] * w[n, idx].to(torch.int64)).sum(1)
    return out


class Ops:
    """Integer operands of (source, N, feature set) on the CPU and the int64 reference of TWICE the epilogue's value
    (alpha = 0.5 gives half-integers), on `dev`.  `lane` salts the seed: lane 0 draws the operands every single-lane
    case has always had, lane 1 an independent set under the same rule (the second lane of a grouped launch), with
    the time-embedding rows in the other order."""

    def __init__(self, src, N, epi, lane=0):
        self.src, self.N, self.epi, self.lane = src, N, epi, lane
        self.f = f = EPI[epi]
        self.B, self.hw, self.M = src_shape(src)
        self.Kd, self.Kreal, self.Kx = src_k(src)
        key = (src, N, epi) if lane == 0 else (src, N, epi, lane)
        gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        B, M = self.B, self.M
        if src[0] == "dense":
            _, self.amode, _, _, _, self.x_wrap, self.f8 = src
            self.s2_shift = 0
            self.a = _sparse_rows(M, self.Kreal, F8_A_NNZ_DENSE if self.f8 else A_NNZ_DENSE, gen)
            self.a_col = self.a
        else:
            _, self.amode, _, self.H, self.W, self.C, _, self.x_wrap, self.f8, self.s2_shift = src
            self.a = _sparse_rows(B * self.H * self.W, self.C, F8_A_NNZ if self.f8 else A_NNZ, gen) \
                .view(B, self.H, self.W, self.C)
            self.a_col = im2col(self.a, self.amode, self.s2_shift).reshape(M, 9 * self.C)
        self.xw = self.x_wrap or self.Kx  # width of X
        ktot = self.Kreal + self.Kx
        w = _weights(N, ktot, gen)
        self.w_main, self.w_x = w[:, :self.Kreal], w[:, self.Kreal:]  # natural order: dense k, conv (tap, c)
        self.x = _sparse_rows(M, self.xw, F8_X_NNZ if self.f8 else X_NNZ, gen) if self.Kx else None
        self.has_bias = not self.f8  # (fp8: the scaled accumulator plus an integer need not fit 8 bits)
        self.bias = torch.randint(-SMALL, SMALL + 1, (N,), generator=gen) if self.has_bias else torch.zeros(N, dtype=torch.int64)
        # fp8: powers of two (1 or 2 per row and per column, 1 .. 4 together); row scales on the dense form only
        self.col_scale = self.row_scale = None
        if self.f8:
            self.col_scale = 2 ** torch.randint(0, 2, (N,), generator=gen)
            self.row_scale = 2 ** torch.randint(0, 2, (M,), generator=gen) if src[0] == "dense" else None
        self.emb = self.emb_row = self.res = None
        if f.get("emb"):  # B + 1 rows, batch element b reads row B - b: row 0 is never read
            self.emb = torch.randint(-SMALL, SMALL + 1, (B + 1, N), generator=gen)
            self.emb_row = torch.tensor([B - b if lane == 0 else b + 1 for b in range(B)], dtype=torch.int32)
        if f.get("res"):
            self.res = torch.randint(-SMALL, SMALL + 1, (M, N), generator=gen)
        self.half = bool(f.get("half"))
        self._ref2: Dict[str, torch.Tensor] = {}

    def w_x_eff(self) -> torch.Tensor:
        """The K-extension's weights per X column: [W_hi | W_lo] both meet the same activation under x_wrap."""
        return self.w_x.to(torch.int64) if not self.x_wrap else \
            self.w_x[:, :self.x_wrap].to(torch.int64) + self.w_x[:, self.x_wrap:].to(torch.int64)

    def acc(self, dev="cpu") -> torch.Tensor:
        """int64 [M, N]: sum_k a w over K and the K-extension."""
        y = int_matmul(self.a_col.to(dev), self.w_main.to(dev))
        if self.Kx:
            y = y + int_matmul(self.x.to(dev), self.w_x_eff().to(dev))
        return y

    def scale(self, dev="cpu") -> torch.Tensor:
        """int64 [M, N] (or 1): the fp8 dequantisation row_scale[m] col_scale[n] the accumulator is multiplied by."""
        if not self.f8:
            return torch.ones((), dtype=torch.int64, device=dev)
        s = self.col_scale.to(dev)[None, :].expand(self.M, self.N)
        return s * self.row_scale.to(dev)[:, None] if self.row_scale is not None else s

    def ref2(self, dev="cpu") -> torch.Tensor:
        """int64 [M, N]: twice the value the epilogue stores, alpha (acc scale + bias) + emb + res."""
        dev = str(dev)
        if dev not in self._ref2:
            y = (1 if self.half else 2) * (self.acc(dev) * self.scale(dev) + self.bias.to(dev))
            if self.emb is not None:
                rows = self.emb[self.emb_row.long()].to(dev)  # [B, N]
                b = torch.arange(self.M, device=dev) // self.hw
                y = y + 2 * rows[b]
            if self.res is not None:
                y = y + 2 * self.res.to(dev)
            self._ref2[dev] = y
        return self._ref2[dev]

    def value(self, dev="cpu") -> torch.Tensor:
        """fp64 [M, N]: the exact output."""
        return self.ref2(dev).double() / 2

    def magnitude(self) -> torch.Tensor:
        """int64 [M, N]: sum_k |a||w| (times the fp8 scale) + |bias| + |emb| + |res|: the exactness bound, <= 256."""
        y = int_matmul(self.a_col.abs(), self.w_main.abs())
        if self.Kx:
            wx = self.w_x.abs().to(torch.int64)
            wx = wx if not self.x_wrap else wx[:, :self.x_wrap] + wx[:, self.x_wrap:]
            y = y + int_matmul(self.x.abs(), wx)
        y = y * self.scale() + self.bias.abs()
        if self.emb is not None:
            y = y + self.emb[self.emb_row.long()].abs()[torch.arange(self.M) // self.hw]
        if self.res is not None:
            y = y + self.res.abs()
        return y

    # -- packing ---------------------------------------------------------------------------------------------------
    def packed_w(self) -> torch.Tensor:
        """[N, Kd_values + Kx] float in the kernel's K order (pack_conv_w of tests/test_kernels_gpu.py for convs; fp8:
        zero-padded to the 128-value K-tile)."""
        from test_kernels_gpu import pack_conv_w
        if self.src[0] == "dense":
            main = self.w_main.float()
        else:
            w4 = self.w_main.view(self.N, 3, 3, self.C).permute(0, 3, 1, 2).float()  # [N, C, 3, 3]
            main = pack_conv_w(w4)[0].float()
        kv = self.Kd * (2 if self.f8 else 1)
        out = torch.zeros(self.N, kv + self.Kx)
        out[:, :main.shape[1]] = main
        out[:, kv:] = self.w_x.float()
        return out

    def fields(self) -> Dict:
        f = dict(M=self.M, N=self.N, K=self.Kd, amode=self.amode, rows_per_b=self.hw, Kx=self.Kx, x_wrap=self.x_wrap,
                 f8=self.f8, s2_shift=self.s2_shift, alpha=0.5 if self.half else 1.0, scale_bias=int(self.half),
                 out_f32=int(bool(self.f.get("out_f32"))), out_split=self.f.get("out_split", 0))
        if self.src[0] == "conv":
            Ho, Wo = out_hw(self.src)
            f.update(C=self.C, Bn=self.B, H=self.H, W=self.W, Ho=Ho, Wo=Wo)
        return f


_OPS: Dict[tuple, Ops] = {}


def operands(case: Case) -> Ops:
    key = (case.src, case.N, case.epi, case.lane)
    if key not in _OPS:
        _OPS[key] = Ops(*key)
    return _OPS[key]


# ---- descriptors -------------------------------------------------------------------------------------------------------
PAD = 32  # padding columns of every operand and output (tests/test_clip_hip_gpu.py _guarded)
PART_CAP = 1 << 23  # split-K workspace (fp32 elements)
SEM_CAP = 1 << 14


def make_desc(**kw):
    from tair_amd import _lib
    d = _lib.GemmDesc()
    d.alpha = 1.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def force_fields(force) -> Dict:
    if force is None:
        return {}
    bm, bn, splits, stages = force
    return dict(force_bm=bm, force_bn=bn, force_splits=splits, force_stages=stages)


def combine_fields(mode: Optional[str], part_ptr, sem_ptr) -> Dict:
    """Every case gets the workspace; coop: tickets (cooperative combine where the grid is resident); last: tickets +
    probe bit 2 (last-arriver combine at any split count); reduce / None: no tickets (the reduce kernel)."""
    kw = dict(partial=part_ptr, partial_cap=PART_CAP)
    if mode in ("coop", "last"):
        kw.update(tile_sem=sem_ptr, sem_cap=SEM_CAP)
    if mode == "last":
        kw.update(probe=4)
    return kw


def leading_dims(o: Ops) -> Dict:
    """lda / ldx / ldw / ld_res / ld_emb / ldo of the guarded buffers (bf16 elements; byte pairs for fp8 A and Wt)."""
    a_cols = o.C if o.src[0] == "conv" else o.Kreal
    ld = dict(lda=(a_cols + PAD) // 2 if o.f8 else a_cols + PAD,
              ldw=(2 * o.Kd + 2 * o.Kx + 2 * PAD) // 2 if o.f8 else o.Kd + o.Kx + 64)
    if o.Kx:
        ld["ldx"] = o.xw + PAD
    if o.res is not None:
        ld["ld_res"] = o.N + PAD
    if o.emb is not None:
        ld["ld_emb"] = o.N + PAD
    ld["ldo"] = (3 * o.N if o.f.get("out_split") else o.N) + PAD
    return ld


def planning_desc(case: Case):
    """The case's descriptor with placeholder pointers: what tair_k_gemm_plan needs (no device)."""
    o = operands(case)
    kw = dict(o.fields(), **leading_dims(o), **force_fields(case.force), **combine_fields(case.combine, 64, 64))
    kw.update(A=64, Wt=64, out=64)
    if o.has_bias:
        kw["bias"] = 64
    if o.Kx:
        kw["X"] = 64
    if o.res is not None:
        kw["res"] = 64
    if o.emb is not None:
        kw.update(emb=64, emb_row=64)
    if o.f8:
        kw["col_scale"] = 64
        if o.row_scale is not None:
            kw["row_scale"] = 64
    if o.f.get("out_lo"):
        kw["out_lo"] = (o.M + 16) * kw["ldo"]
    return make_desc(**kw)


def plan_of(d) -> Tuple[int, Tuple[int, int, int, int]]:
    """(status, (kernel, bm, bn, splits)) of tair_k_gemm_plan: host only."""
    from tair_amd import _lib
    out = [ctypes.c_int() for _ in range(4)]
    rc = _lib.lib().tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(x) for x in out])
    bm, bn, splits, kern = (x.value for x in out)
    return rc, (kern, bm, bn, splits)


# the forced plans of the all-plans-agree test: every family, unsplit and in two slices
ALL_PLANS = [(bm, bn, s, T3) for bm, bn in TILES for s in (1, 2)] + \
            [(-bm, bn, s, 0) for bm, bn in RINGS for s in (1, 2)] + [(bm, bn, 1, 4) for bm, bn in PHASES] + \
            [(bm, bn, 1, 2) for bm, bn in SHALLOWS] + [(64, bn, s, 100 + st) for bn, st in DEEPS for s in (1, 2)] + \
            [(bm, bn, s, 203) for bm, bn in KGROUPS for s in (1, 2)] + \
            [(256, bn, s, 9) for bn in (64, 128, 160, 192) for s in (1, 2)]
# (descriptor, the number of ALL_PLANS that accept it): dense takes all but the halo tiles; a stride-1 conv all but
# the shallow and the halo tiles; a 16-wide conv without K-extension also the three halo widths built for it
AGREE = [
    (Case("agree-dense-m257n200k320x64", dense(257, 320, 64), 200, "ber", None, None), len(ALL_PLANS) - 8),
    (Case("agree-conv2x8x16c128n200x64", conv(A_CONV3, 2, 8, 16, 128, 64), 200, "ber", None, None),
     len(ALL_PLANS) - 8 - 2),
    (Case("agree-conv2x16x16c128n72", conv(A_CONV3, 2, 16, 16, 128), 72, "br", None, None), len(ALL_PLANS) - 2 - 2),
]


# ---- two lanes in one launch (tair_k_gemm_grouped) ---------------------------------------------------------------------
class GroupCase:
    """Two same-shape GEMMs / convs as lanes 0 and 1 of ONE launch (a UNet layer and the same ControlNet layer in the
    product).  The lanes share the source, N, the forced plan, the combine and the output kind (out_f32, out_split,
    operand type), as the launcher demands; their feature sets epis[0] | epis[1] may differ -- epilogue_tile picks its
    features per tile from that tile's lane.  Lane i's operands are Ops(src, N, epis[i], lane=i): an independent draw
    under the same rule.  expect is the plan of TWO lanes (tair_k_gemm_plan_lanes); expect_one, where given, the plan
    the same request gets alone (the planner's own plans that differ)."""

    def __init__(self, name, src, N, epis, force, expect, combine=None, expect_one=None, tags=()):
        self.name, self.src, self.N, self.epis, self.force = name, src, N, tuple(epis), force
        self.expect, self.combine, self.expect_one, self.tags = tuple(expect), combine, expect_one, frozenset(tags)

    @property
    def is_conv(self):
        return self.src[0] == "conv"

    def lane(self, i) -> Case:
        return Case(f"{self.name}[lane {i}]", self.src, self.N, self.epis[i], self.force, self.expect, self.combine,
                    lane=i)

    def workgroups(self) -> int:
        """tiles_m * 2 * tiles_n * splits of the main kernel's grid."""
        _, bm, bn, splits = self.expect
        return cdiv(src_shape(self.src)[2], abs(bm)) * 2 * cdiv(self.N, bn) * splits

    def __repr__(self):
        return self.name


def src_name(src) -> str:
    if src[0] == "dense":
        _, _, M, K, Kx, xw, f8 = src
        return ("f8" if f8 else "") + f"dense-m{M}k{K}" + (f"x{Kx}" if Kx else "") + ("w" if xw else "")
    _, amode, B, H, W, C, Kx, xw, f8, sh = src
    kind = {A_CONV3: "conv", A_CONV3_S2: "s2conv", A_CONV3_UP: "upconv", A_SMALLC: "smallc"}[amode]
    return ("f8" if f8 else "") + f"{kind}{B}x{H}x{W}c{C}" + (f"x{Kx}" if Kx else "") + ("w" if xw else "") + \
        (f"-shift{sh}" if amode == A_CONV3_S2 else "")


GROUP_CASES: List[GroupCase] = []
# mixed pairs both ways round, then pairs of one feature set (whose two lanes still differ in every operand)
G_MIXED = (("b", "ber"), ("br", "b"), ("lo", "br"), ("half", "b"), ("ber", "b"), ("b", "br"), ("br", "lo"),
           ("b", "half"))
G_PAIRS = G_MIXED + (("be", "ber"), ("f32", "half32"), ("sp1", "sp1"), ("sp2", "sp2"), ("half32", "f32"), ("lo", "lo"))
G_PAIRS_HALO = (("b", "ber"), ("br", "b"), ("lo", "br"), ("ber", "b"), ("f32", "f32"), ("br", "lo"))  # H_EPI's sets
G_PAIRS_F8 = (("b", "br"), ("lo", "br"), ("f32", "f32"), ("br", "b"))  # F8_EPI's sets
G_M, G_N = (63, 130, 257), (70, 200)  # tiles_m 1 / 3 / 5 at 64 rows, 1 / 2 / 3 at 128, 1 / 1 / 2 at 256


def _gkind(force):
    if force is None:
        return "own"
    bm, bn, _, st = force
    kind = "kgroup" if st >= 200 else f"deep-s{st - 100}-" if st >= 100 else "halo" if st == 9 else "phase" if st == 4 \
        else "shallow" if st == 2 else "ring" if bm < 0 else "tile"
    return f"{kind}{abs(bm)}x{bn}"


def _gadd(src, N, pair, force, combine=None, expect=None, expect_one=None, tags=()):
    if expect is None:
        expect = expect_forced(src, force)
    if expect[3] == 1 and force is not None:
        combine = None
    name = f"g-{_gkind(force)}-{src_name(src)}-n{N}-s{expect[3]}" + (f"-{combine}" if combine and expect[3] > 1 else "") + \
        f"-{pair[0]}+{pair[1]}"
    GROUP_CASES.append(GroupCase(name, src, N, pair, force, expect, combine, expect_one, tags))


_G_FAMILIES = [(bm, bn, T3) for bm, bn in ((64, 64), (64, 128), (128, 128), (128, 320), (256, 128), (256, 160))] + \
              [(-64, 64, 0), (-128, 256, 0), (-256, 128, 0), (64, 64, 104), (64, 64, 108), (64, 64, 203), (64, 128, 203),
               (256, 256, 4), (256, 320, 4), (64, 64, 2), (64, 128, 2)]
# -- every family unsplit: dense, (M, N) running through all six combinations, the K-extension and the pairs rotating
for _i, (_bm, _bn, _st) in enumerate(_G_FAMILIES):
    _Kx = (0, 64, 0, 128)[_i % 4]
    _gadd(dense(G_M[_i % 3], 160 if _bm < 0 else 192, _Kx, 64 if _Kx == 128 else 0), G_N[_i % 2], G_PAIRS[_i % len(G_PAIRS)],
          (_bm, _bn, 1, _st), tags=("family",))
# -- every family that splits, split: the reduce kernel everywhere, the in-kernel combines on the 64-row tiles
for _i, (_bm, _bn, _st) in enumerate(_G_FAMILIES):
    if _st in (4, 2):
        continue  # (the 4-phase kernel and the 2-stage tiles never split)
    _modes = ("coop", "last", "reduce") if (abs(_bm) == 64 and _bm > 0 and not 100 <= _st < 200) else \
        ("last", "reduce") if 100 <= _st < 200 else ("reduce",)
    for _j, _mode in enumerate(_modes):
        _src, _N = ((SPLIT_SRC, 200), (SPLIT_SRC_X, 70))[(_i + _j) % 2]
        _gadd(_src, _N, G_PAIRS[(_i + 3 * _j + 5) % len(G_PAIRS)], (_bm, _bn, 3 if _bm < 0 else 2, _st), _mode,
              tags=("family",))
# -- the lane boundary under xcd_remap: tiles_m 1 / 3 / 5 with two and four n-tiles, unsplit and in three slices with
# the cooperative order (modes 3 / 4): tiles_m * 2 * tiles_n * splits is a multiple of 8 for some and not for others
for _i, (_M, _N) in enumerate((m, n) for m in G_M for n in G_N):
    _gadd(dense(_M, 320), _N, G_MIXED[_i % 8], (64, 64, 1, T3), tags=("boundary",))
    _gadd(dense(_M, 320), _N, G_MIXED[(_i + 3) % 8], (64, 64, 3, T3), "coop", tags=("boundary",))
    _gadd(dense(_M, 320), _N, G_MIXED[(_i + 5) % 8], (128, 128, 2, T3), "reduce", tags=("boundary",))
# -- every combine at 2, 3 and 5 slices, dense (five K-tiles) and conv (ten)
for _i, _s in enumerate((2, 3, 5)):
    for _j, _mode in enumerate(("coop", "last", "reduce")):
        _gadd(SPLIT_SRC, 200, G_PAIRS[(3 * _i + _j) % len(G_PAIRS)], (64, 64, _s, T3), _mode, tags=("combine",))
        _gadd(SPLIT_SRC_X, 70, G_PAIRS[(3 * _i + _j + 4) % len(G_PAIRS)], (64, 128, _s, T3), _mode, tags=("combine",))
        _gadd(CS_SRC, 72, G_MIXED[(3 * _i + _j) % 8], (64, 64, _s, T3), _mode, tags=("combine",))
# -- conv sources: stride 1 (C = 64 / 192, with and without the K-extension, x_wrap), stride 2 at both shifts, the
# fused upsample, the small-channel mode, halo tiles at the three widths, fp8
for _i, ((_B, _H, _W), _C, (_Kx, _xw)) in enumerate((((3, 5, 7), 64, (0, 0)), ((2, 8, 16), 192, (64, 0)),
                                                      ((1, 30, 24), 64, (128, 64)), ((3, 5, 7), 192, (64, 0)),
                                                      ((2, 8, 16), 64, (128, 64)), ((1, 30, 24), 192, (0, 0)))):
    _force = ((64, 64, 1, T3), (128, 128, 1, T3), (-128, 256, 1, 0), (64, 64, 1, 104), (64, 128, 1, 203),
              (256, 320, 1, 4))[_i]
    _gadd(conv(A_CONV3, _B, _H, _W, _C, _Kx, _xw), (72, 200)[_i % 2], G_PAIRS[(2 * _i) % len(G_PAIRS)], _force,
          tags=("conv1",))
_gadd(CS_SRC, 72, ("ber", "b"), (128, 128, 3, T3), "reduce", tags=("conv1",))
_gadd(CS_SRC, 72, ("lo", "br"), (64, 64, 3, 203), "coop", tags=("conv1",))
for _sh in (0, 1):
    _gadd(conv(A_CONV3_S2, 2, 8, 16, 64, 0, 0, 0, _sh), 72, G_MIXED[_sh], (64, 64, 1, T3), tags=("s2",))
    _gadd(conv(A_CONV3_S2, 2, 8, 16, 128, 0, 0, 0, _sh), 200, G_MIXED[2 + _sh], (64, 128, 2, T3), "reduce", tags=("s2",))
_gadd(conv(A_CONV3_UP, 2, 4, 8, 64), 72, ("b", "ber"), (64, 64, 1, T3), tags=("up",))
_gadd(conv(A_CONV3_UP, 2, 4, 8, 128), 200, ("br", "b"), (64, 128, 3, T3), "coop", tags=("up",))
_gadd(conv(A_SMALLC, 2, 8, 16, 8), 72, ("lo", "br"), (64, 64, 1, T3), tags=("smallc",))
_gadd(conv(A_SMALLC, 3, 5, 7, 8), 64, ("half", "b"), (64, 128, 2, T3), "reduce", tags=("smallc",))  # 72 -> 2 K-tiles
for _i, (_B, _H, _W) in enumerate(((1, 16, 16), (2, 32, 16), (1, 8, 32), (1, 64, 64))):
    _bn = HALO_BN[_W][_i % 3]
    _gadd(conv(A_CONV3, _B, _H, _W, 192), (72, 200, 64, 72)[_i], G_PAIRS_HALO[_i], (256, _bn, 1, 9), tags=("halo",))
    _gadd(conv(A_CONV3, _B, _H, _W, 192), (200, 72, 72, 64)[_i], G_PAIRS_HALO[(_i + 2) % 6], (256, _bn, (3, 2, 3, 2)[_i], 9),
          "reduce", tags=("halo",))
_gadd(dense(65, 128, 0, 0, 1), 70, G_PAIRS_F8[0], (64, 64, 1, 0), tags=("f8",))
_gadd(dense(257, 640, 0, 0, 1), 200, G_PAIRS_F8[1], (64, 64, 2, 0), "last", tags=("f8",))
_gadd(dense(257, 384, 0, 0, 1), 200, G_PAIRS_F8[2], (128, 128, 3, 0), "reduce", tags=("f8",))
_gadd(conv(A_CONV3, 2, 8, 16, 64, 0, 0, 1), 70, G_PAIRS_F8[3], (64, 64, 1, 0), tags=("f8",))
_gadd(conv(A_CONV3, 3, 5, 7, 128, 64, 0, 1), 200, G_PAIRS_F8[0], (128, 128, 2, 0), "reduce", tags=("f8",))
# -- the planner's own plans where two lanes plan differently from one (gemm_plan / kgroup_rule, by hand)
# dense 257 x 200 x 320 with a K-extension of 64 (the composite FF-out rule): 5 x 4 = 20 tiles of 64 x 64, 6 K-tiles.
#   One lane: no slice count c with 6 / c >= 10: unsplit.  Two lanes: (200 + 10) / 20 = 10 slices, capped at
#   2 * 6 / 5 = 2; a dense GEMM never takes the two-K-group form by rule
_gadd(dense(257, 320, 64), 200, ("lo", "br"), None, "coop", (K_TILE, 64, 64, 2), (K_TILE, 64, 64, 1), tags=("own",))
# conv 1 x 30 x 24, C = 64 -> N = 72: BNc = 64, 12 x 2 = 24 tiles, (400 + 12) / 24 = 17 slices capped at 9 / 3 = 3.
#   One lane: 24 < 32 tiles, no two-K-group plan (kgroup_rule).  Two lanes: 48 tiles in [32, 256], 48 * 3 <= 512,
#   one image, tickets: min(256 / 48, 9 / 15) = 0 -> one slice of 9 >= 4 K-tiles: the two-K-group kernel, unsplit
_gadd(conv(A_CONV3, 1, 30, 24, 64), 72, ("be", "ber"), None, "coop", (K_KGROUP, 64, 64, 1), (K_TILE, 64, 64, 3),
      tags=("own",))
# -- the blocked workgroup order (xcd_remap mode 5) with two lanes.  The host rule (gemm.hip): dense, one slice, a
# 3-stage tile; with gx = 2 * tiles_m and gy = tiles_n: gx * gy > 512, weights gy * bn * K * 2 bytes > 2 MiB, and a block
# of bmr x bnc tiles (bmr | gx, bnc | gy, 16 <= bmr * bnc <= 64, (gx / bmr) * (gy / bnc) % 8 == 0) whose traffic
# ab * gy / bnc + wb * gx / bmr is below 0.7 x the better of the two plain orders (blocked_pick below is that rule).
# On the smallest tile, 64 x 64, with M = 130 (tiles_m = 3: gx = 6, so a block of bmr = 2 rows holds the last m-tile of
# lane 0 and the first of lane 1), N = 6 (mod 64) as the other cases and K a multiple of 64 with more than one K-tile:
# gy >= 86 for the grid, and the weights need gy * 64 * K > 2^20; the smallest weight matrix that also has an admissible
# block is K = 192, gy = 88 (N = 5574, block 2 x 11: 3 x 8 = 24 blocks); gy = 86, 87 have no divisor pair that
# passes.  One lane of the same shape has gx * gy = 264 <= 512 and keeps the plain order.
BLOCKED = (130, 5574, 192)
_gadd(dense(BLOCKED[0], BLOCKED[2]), BLOCKED[1], ("b", "br"), (64, 64, 1, T3), tags=("blocked",))

GROUP_CASE = {c.name: c for c in GROUP_CASES}
assert len(GROUP_CASE) == len(GROUP_CASES), [c.name for c in GROUP_CASES if sum(d.name == c.name for d in GROUP_CASES) > 1]


def blocked_pick(M, N, K, bm, bn, lanes) -> Tuple[int, int]:
    """(bmr, bnc) of the blocked order gemm_grouped picks for a dense one-slice bm x bn tile plan of `lanes` lanes, or
    (0, 0): the rule of gemm.hip, re-stated."""
    gx, gy = cdiv(M, bm) * lanes, cdiv(N, bn)
    wb, ab = bn * K * 2.0 * gy, M * K * 2.0 * lanes
    if not (gx * gy > 512 and wb > (2 << 20)):
        return 0, 0
    best, pick = min(ab + wb * gx, ab * gy + wb), (0, 0)
    for bnc in range(1, 17):
        for bmr in range(1, 17):
            if gy % bnc or gx % bmr or not 16 <= bmr * bnc <= 64 or ((gx // bmr) * (gy // bnc)) % 8:
                continue
            c = ab * (gy // bnc) + wb * (gx // bmr)
            if c < 0.7 * best:
                best, pick = c, (bmr, bnc)
    return pick


def pair_descs(gc: GroupCase, ptrs=None):
    """The two descriptors of a pair as one ctypes array (what tair_k_gemm_grouped takes).  ptrs: per lane the
    descriptor fields of its device buffers (tests/test_grouped_exact_gpu.py); None: placeholder pointers, which is
    all the plan query and the dry check read."""
    from tair_amd import _lib
    arr = (_lib.GemmDesc * 2)()
    for i in range(2):
        d = planning_desc(gc.lane(i)) if ptrs is None else make_desc(**ptrs[i])
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(d), ctypes.sizeof(_lib.GemmDesc))
    return arr


def plan_of_lanes(d, lanes) -> Tuple[int, Tuple[int, int, int, int]]:
    """(status, (kernel, bm, bn, splits)) of tair_k_gemm_plan_lanes: host only."""
    from tair_amd import _lib
    out = [ctypes.c_int() for _ in range(4)]
    rc = _lib.lib().tair_k_gemm_plan_lanes(ctypes.byref(d), lanes, *[ctypes.byref(x) for x in out])
    bm, bn, splits, kern = (x.value for x in out)
    return rc, (kern, bm, bn, splits)


def swapped_ref2(o: Ops, other: Ops, what: str) -> Optional[torch.Tensor]:
    """o's reference with ONE per-lane operand taken from the other lane (what a single mixed-up pointer computes), or
    None where either lane has no such operand.  what: a, w, x, bias, emb, emb_row, res, col_scale, row_scale."""
    import copy
    fields = {"a": ("a", "a_col"), "w": ("w_main", "w_x"), "bias": ("bias",)}.get(what, (what,))
    if any(getattr(o, f) is None or getattr(other, f) is None for f in fields) or (what == "bias" and not o.has_bias):
        return None
    m = copy.copy(o)
    m._ref2 = {}
    for f in fields:
        setattr(m, f, getattr(other, f))
    return m.ref2()


SWAPS = ("a", "w", "x", "bias", "emb", "emb_row", "res", "col_scale", "row_scale")


# ---- attention ---------------------------------------------------------------------------------------------------------
KT = 64
A_SQ = (1, 15, 17, 63, 65, 100, 129)
A_SKV = (1, 63, 64, 65, 77, 130, 257, 1000)
WS_BIG = 64 << 20


class AttnCase:
    """api: plain (tair_k_attention), ex (tair_k_attention_ex) or tk (tair_k_attention_tk); force (qsets, splits);
    ws_bytes of the workspace handed over (0: none); layout: rows (q, k, v in buffers of their own), shared (one
    context for all batch elements, kv_bstride = 0) or fused (strided out of one [T, 3C] buffer, Sq == Skv);
    expect: the effective (qsets, splits, kv_split)."""

    def __init__(self, name, B, H, Sq, Skv, api, force, ws_bytes, expect, layout="rows"):
        self.name, self.B, self.H, self.Sq, self.Skv, self.api = name, B, H, Sq, Skv, api
        self.force, self.ws_bytes, self.expect, self.layout = force, ws_bytes, tuple(expect), layout

    def __repr__(self):
        return self.name


def attn_per_split(B, H, Sq) -> int:
    return B * Sq * H * (64 * 2 + 8)


def attn_expect(B, H, Sq, Skv, force, ws_bytes) -> Tuple[int, int, int]:
    """attention_plan (tair_amd/csrc/attention.hip) for these small shapes: the heuristic keeps 16 queries per wave
    below 256 query blocks and never splits below 32 key tiles; a forced split count is clamped to the key tiles and
    to the workspace, then evened out (ceil(tiles / splits) tiles per split, no empty split)."""
    qsets, fs = force
    ktiles = cdiv(Skv, KT)
    assert cdiv(Sq, 64) * B * H < 256 and ktiles < 32
    q = qsets or 1
    s = max(1, min(fs, ktiles)) if fs else 1
    if s > 1 and attn_per_split(B, H, Sq) * s > ws_bytes:
        s = max(1, ws_bytes // attn_per_split(B, H, Sq))
    tps = cdiv(ktiles, s)
    return q, cdiv(ktiles, tps), tps * KT


def _last_partial(Skv):
    """A forced split count that leaves the last split a single partial tile (or 2 where Skv has no partial tile / one
    tile only)."""
    ktiles = cdiv(Skv, KT)
    for s in range(2, ktiles + 1):
        tps = cdiv(ktiles, s)
        if (ktiles - 1) % tps == 0 and Skv % KT and cdiv(ktiles, tps) > 1:
            return s
    return 2


ATTN_OPTS = ("plain", "ex-q1-s1", "ex-q2-s2", "tk-q1-partial", "tk-q2-above", "ex-q1-smallws", "tk-q2-s2")
ATTN_CASES: List[AttnCase] = []
for _i, _Skv in enumerate(A_SKV):
    for _j, _opt in enumerate(ATTN_OPTS):
        _Sq = A_SQ[(_i + _j) % 7]
        _B, _H = (1, 3)[(_i + _j) % 2], (1, 2, 5)[(_i + 2 * _j) % 3]
        _kt = cdiv(_Skv, KT)
        _ws = WS_BIG
        if _opt == "plain":
            _api, _force, _ws = "plain", (0, 0), 0
        elif _opt == "ex-q1-s1":
            _api, _force = "ex", (1, 1)
        elif _opt in ("ex-q2-s2", "tk-q2-s2"):
            _api, _force = _opt[:2], (2, 2)
        elif _opt == "tk-q1-partial":
            _api, _force = "tk", (1, _last_partial(_Skv))
        elif _opt == "tk-q2-above":
            _api, _force = "tk", (2, _kt + 3)
        else:  # a workspace of two splits (and a bit) under a forced count of four
            _api, _force, _ws = "ex", (1, 4), 2 * attn_per_split(_B, _H, _Sq) + 100
        ATTN_CASES.append(AttnCase(f"attn-b{_B}h{_H}q{_Sq}k{_Skv}-{_opt}", _B, _H, _Sq, _Skv, _api, _force, _ws,
                                   attn_expect(_B, _H, _Sq, _Skv, _force, _ws)))
ATTN_CASES += [
    AttnCase("attn-b3h2q100k77-shared-plain", 3, 2, 100, 77, "plain", (0, 0), 0, (1, 1, 128), "shared"),
    AttnCase("attn-b3h5q17k257-shared-tk-s3", 3, 5, 17, 257, "tk", (1, 3), WS_BIG, (1, 3, 128), "shared"),
    AttnCase("attn-b3h2q65k65-fused-plain", 3, 2, 65, 65, "plain", (0, 0), 0, (1, 1, 128), "fused"),
    AttnCase("attn-b1h5q130k130-fused-tk-s2", 1, 5, 130, 130, "tk", (2, 2), WS_BIG, (2, 2, 128), "fused"),
    # a workspace below one split's partials: no split at all
    AttnCase("attn-b1h2q63k257-ex-nows", 1, 2, 63, 257, "ex", (1, 3), 1000, (1, 1, 320)),
]
ATTN_CASE = {c.name: c for c in ATTN_CASES}
assert len(ATTN_CASE) == len(ATTN_CASES)


def attn_plan_of(c: AttnCase) -> Tuple[int, Tuple[int, int, int]]:
    """(status, effective (qsets, splits, kv_split)) from the library: tair_k_attention_plan for the unforced API,
    tair_k_attention_plan_ex for the forced ones (host only)."""
    from tair_amd import _lib
    out = [ctypes.c_int() for _ in range(3)]
    refs = [ctypes.byref(x) for x in out]
    if c.api == "plain":
        rc = _lib.lib().tair_k_attention_plan(c.B, c.H, c.Sq, c.Skv, 0, *refs)
    else:
        rc = _lib.lib().tair_k_attention_plan_ex(c.B, c.H, c.Sq, c.Skv, c.ws_bytes, c.force[0], c.force[1], *refs)
    return rc, tuple(x.value for x in out)


def hadamard64() -> torch.Tensor:
    h = torch.ones(1, 1)
    while h.shape[0] < 64:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    return h


def required_targets(Skv, splits, kv_split) -> List[int]:
    """Key 0, keys 63 and 64, the last key of every key tile and the first of the next, the first and last key of
    every split, key Skv - 1."""
    req = {0, Skv - 1}
    for t in range(KT, Skv, KT):
        req |= {t - 1, t}
    for s in range(splits):
        req |= {s * kv_split, min(Skv, (s + 1) * kv_split) - 1}
    return sorted(k for k in req if 0 <= k < Skv)


class AttnOps:
    """One-hot operands of a case under its effective plan: per (batch, head) the target set (the required keys plus
    random others, at most 64), q / k / v [B, S, H, 64] (float holding bf16 values) and tgt [B, H, Sq], the key each
    query selects.  A shared context (kv_bstride = 0) has one k / v / target set per head for all batch elements.
    `lane` salts the seed (lane 0: the operands every single-lane case has always had): the second lane of a grouped
    launch gets target sets, Hadamard rows and V of its own."""

    def __init__(self, c: AttnCase, lane=0):
        B, H, Sq, Skv = c.B, c.H, c.Sq, c.Skv
        gen = torch.Generator().manual_seed(zlib.crc32((c.name if lane == 0 else f"{c.name}#lane{lane}").encode()))
        had = hadamard64()
        req = required_targets(Skv, c.expect[1], c.expect[2])
        assert len(req) <= 64
        Bk = 1 if c.layout == "shared" else B
        self.Bk = Bk
        self.k = torch.zeros(Bk, Skv, H, 64)
        self.v = torch.randn(Bk, Skv, H, 64, generator=gen).to(torch.bfloat16).float()
        self.q = torch.zeros(B, Sq, H, 64)
        self.tgt = torch.zeros(B, H, Sq, dtype=torch.long)
        self.sets: Dict[Tuple[int, int], List[int]] = {}
        for bk in range(Bk):
            for h in range(H):
                others = [k for k in torch.randperm(Skv, generator=gen).tolist() if k not in req][:64 - len(req)]
                T = req + sorted(others)
                rows = torch.randperm(64, generator=gen)[:len(T)]
                self.k[bk, T, h] = had[rows]
                self.sets[(bk, h)] = T
                for b in (range(B) if Bk == 1 else [bk]):
                    j = (torch.arange(Sq) + 7 * b + 3 * h) % len(T)
                    self.q[b, :, h] = 32 * had[rows[j]]
                    self.tgt[b, h] = torch.tensor(T)[j]

    def expected(self) -> torch.Tensor:
        """[B, Sq, H, 64]: V[t(i)]."""
        B, Sq, H = self.q.shape[:3]
        out = torch.zeros(B, Sq, H, 64)
        for b in range(B):
            for h in range(H):
                out[b, :, h] = self.v[b if self.Bk > 1 else 0, self.tgt[b, h], h]
        return out


# ---- two attention lanes in one launch (tair_k_attention_grouped) ------------------------------------------------------
# mode: unsplit; split (no tickets: attn_combine_kernel, lane = blockIdx.y); tk (tickets: merged in-kernel, lane from
# blockIdx.z / nsplit).  Every lane has its own workspace and tickets (tests/test_grouped_kernels_gpu.py).
G_ATTN_SQ, G_ATTN_SKV, G_ATTN_BH = (17, 65, 129), (77, 130, 257), ((1, 2), (3, 1), (2, 2))
GROUP_ATTN_CASES: List[AttnCase] = []
for _i, _Sq in enumerate(G_ATTN_SQ):
    for _j, _Skv in enumerate(G_ATTN_SKV):
        for _m, _mode in enumerate(("unsplit", "split", "tk")):
            _B, _H = G_ATTN_BH[(_i + _j + _m) % 3]
            _layout = "shared" if (_i + _j + _m) % 2 and _B > 1 else "rows"
            _force = ((1, 2)[(_i + _j) % 2], 1 if _mode == "unsplit" else (2, 3, 5)[(_i + _m) % 3])
            GROUP_ATTN_CASES.append(AttnCase(f"gattn-b{_B}h{_H}q{_Sq}k{_Skv}-{_layout}-q{_force[0]}-{_mode}{_force[1]}", _B, _H,
                                             _Sq, _Skv, _mode, _force, WS_BIG, attn_expect(_B, _H, _Sq, _Skv, _force, WS_BIG),
                                             _layout))
assert len({c.name for c in GROUP_ATTN_CASES}) == len(GROUP_ATTN_CASES)
