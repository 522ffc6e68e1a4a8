"""GroupNorm statistics epilogues at the UNet's group geometry: operands, fp64 references and the case table shared
by tests/test_gn_stats_cpu.py (every case resolves to the plan it names: no device) and tests/test_gn_stats_gpu.py
(each case against fp64 on the device).

A case is a producer GEMM (dense, or a 3x3 conv in one of the loader modes) with an epilogue feature set, one or two
statistics targets (group width cg, G groups, channel offset c_off inside the normalised tensor) and a plan: forced
through force_bm / force_bn / force_splits / force_stages, or the planner's own.  `expect` is the (kernel, bm, bn,
splits) that gemm_grouped (tair_amd/csrc/gemm.hip) resolves the request to, derived from its rules by hand:

* a forced tile is kept, except that with statistics a tile must not straddle two batch elements: bm is halved
  until it divides hw (or reaches 64), and where the halved tile is not built (gemm_tile_built / gemm_ring_built)
  bn becomes 128;
* the 4-phase kernel needs hw % 256 == 0, otherwise the request becomes a tile-kernel plan with bn = 128 (and is
  then halved as above);
* one batch element (M == hw) may have any hw: rows past M take no part in the sums;
* the planner's own small-grid rule: 64-row tiles, 128 columns for convs with N >= 256 (64 for stride-2 convs up to
  640 channels), K split toward 400 (480) workgroups with >= 3 K-tiles per slice; a one-image stride-1 conv with
  32 .. 256 tiles and tickets takes the two-K-group kernel with min(256 / tiles, K-tiles / 15) >= 1 slices.

Inputs make every (batch element, group) sum distinct: the batch elements' activations have means MU (|mean| >= 2
std) against weights of positive mean, the time-embedding rows differ per batch element and are indexed through a
permuting emb_row, and the bias is a ramp over the channels.  A sum that lands in another batch element's slot or in
a neighbouring group is off by far more than any bound below.
"""
import ctypes
import zlib
from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

A_DENSE, A_CONV3, A_CONV3_S2, A_CONV3_UP, A_SMALLC = 0, 1, 2, 3, 4
K_TILE, K_PHASE, K_SHALLOW, K_HALO, K_DEEP, K_KGROUP = 0, 1, 2, 3, 4, 5
STAT_REPL = 8
G = 32  # GroupNorm groups of the UNet

Tgt = namedtuple("Tgt", "cg G c_off")

# output channels N and the statistics targets of the UNet's producers
GEOM: Dict[str, Tuple[int, List[Tgt]]] = {
    "n320": (320, [Tgt(10, G, 0)]),                          # a 320-channel norm
    "skip320": (320, [Tgt(10, G, 0), Tgt(30, G, 640)]),      # ... whose output is also the skip of cat([h640, skip])
    "h640of960": (640, [Tgt(30, G, 0)]),                     # h of that concat: groups 0 .. 21, group 21 partly
    "n640": (640, [Tgt(20, G, 0)]),
    "skip640": (640, [Tgt(20, G, 0), Tgt(60, G, 1280)]),     # skip of cat([h1280, skip640]): 1920 channels
    "h1280of1920": (1280, [Tgt(60, G, 0)]),
    "n1280": (1280, [Tgt(40, G, 0)]),
    "lo2560": (1280, [Tgt(80, G, 0)]),                       # first half of a 2560-channel norm
    "hi2560": (1280, [Tgt(80, G, 1280)]),                    # second half
}

# epilogue feature sets: (time embedding, hi + lo residual, second output plane, act)
EPI = {
    "emb": dict(emb=True),                 # bias + emb + stats (listed): ResBlock conv1
    "reslo": dict(res=True, out_lo=True),  # bias + hi/lo residual + out_lo + stats [+ stats2] (listed)
    "outlo": dict(out_lo=True),            # bias + out_lo + stats [+ stats2] (listed)
    "plain": dict(),                       # bias + stats [+ stats2] on a plain bf16 output (generic loop)
    "silu": dict(act=1),                   # SiLU + stats (generic loop)
}

MU = (3.0, -4.0, 2.0, -2.5)  # activation mean per batch element (std 1)


class Case:
    def __init__(self, name, src, geom, epi, force, expect, combine=None, stands_for=""):
        self.name, self.src, self.geom, self.epi = name, src, geom, epi
        self.force, self.expect, self.combine, self.stands_for = force, tuple(expect), combine, stands_for
        self.N, self.targets = GEOM[geom]

    @property
    def hilo(self) -> bool:
        return bool(EPI[self.epi].get("out_lo"))

    @property
    def listed_two_target(self) -> bool:
        """A listed feature set with E_STATS2 (TAIR_EPI_LISTED): the probe = 0 / probe = 4 comparison applies."""
        return self.epi in ("reslo", "outlo") and len(self.targets) == 2 and self.expect[3] == 1

    def __repr__(self):
        return self.name


# ---- operand sources ------------------------------------------------------------------------------------
def dense(B, hw, K, Kx=0):
    return ("dense", B, hw, K, Kx)


def conv(amode, B, H, W, C, Kx=0):
    return ("conv", amode, B, H, W, C, Kx)


D2 = dense(2, 256, 192)        # M = 512, three K-tiles
D2K64 = dense(2, 256, 64)
D2X = dense(2, 256, 128, 64)   # with a K-extension (the composite proj_out, a 1x1 skip conv)
C2 = conv(A_CONV3, 2, 16, 16, 64)       # M = 512, hw = 256, nine K-tiles
C2X = conv(A_CONV3, 2, 16, 16, 64, 64)  # conv2 with the skip conv as the K-extension
C2C128 = conv(A_CONV3, 2, 16, 16, 128)  # two 64-channel chunks (the halo split)
C2W64 = conv(A_CONV3, 2, 4, 64, 64)     # 64-wide image rows, hw = 256
DHW64 = dense(4, 64, 128)      # B = 4, M = 256: 128- and 256-row tiles must shrink
DHW320 = dense(2, 320, 64)     # hw % 256 != 0
C900 = conv(A_CONV3, 1, 30, 30, 64)     # B = 1, M = hw = 900: ragged rows
S2 = conv(A_CONV3_S2, 2, 32, 32, 64)    # -> 16 x 16
UP = conv(A_CONV3_UP, 2, 8, 8, 64)      # -> 16 x 16
SMALLC = conv(A_SMALLC, 2, 16, 16, 4)


def src_shape(src):
    """(B, hw, M) of a source's output."""
    if src[0] == "dense":
        return src[1], src[2], src[1] * src[2]
    _, amode, B, H, W, _, _ = src
    hw = (H // 2) * (W // 2) if amode == A_CONV3_S2 else 4 * H * W if amode == A_CONV3_UP else H * W
    return B, hw, B * hw


def _c(name, src, geom, epi, force, expect, combine=None, stands_for=""):
    return Case(name, src, geom, epi, force, expect, combine, stands_for)


T3 = 3  # force_stages: the 3-stage tile kernels
CASES: List[Case] = [
    # ---- kernel 0, the tile kernels: 4-wave 64 / 128-row tiles and the 8-wave 128 x 256 / 128 x 320 / 256 x 128
    _c("tile64x64-dense", D2, "skip320", "outlo", (64, 64, 1, T3), (K_TILE, 64, 64, 1)),
    _c("tile64x128-dense", D2X, "skip640", "reslo", (64, 128, 1, T3), (K_TILE, 64, 128, 1), None,
       "composite proj_out (K-extension, hi + lo residual), skip of the 1920-channel concat"),
    _c("tile128x128-dense", D2, "skip320", "plain", (128, 128, 1, T3), (K_TILE, 128, 128, 1)),
    _c("tile128x256-dense", D2, "n1280", "emb", (128, 256, 1, T3), (K_TILE, 128, 256, 1)),
    _c("tile128x320-dense", D2, "skip640", "outlo", (128, 320, 1, T3), (K_TILE, 128, 320, 1)),
    _c("tile256x128-dense", D2, "lo2560", "silu", (256, 128, 1, T3), (K_TILE, 256, 128, 1)),
    _c("tile64x64-conv", C2, "n320", "emb", (64, 64, 1, T3), (K_TILE, 64, 64, 1), None, "ResBlock conv1 (B >= 2)"),
    _c("tile64x128-conv", C2X, "hi2560", "outlo", (64, 128, 1, T3), (K_TILE, 64, 128, 1), None,
       "ResBlock conv2 with the skip K-extension"),
    _c("tile128x128-conv", C2, "h640of960", "reslo", (128, 128, 1, T3), (K_TILE, 128, 128, 1), None,
       "ResBlock conv2 without the skip K-extension (trunk residual), h of the 960-channel concat"),
    _c("tile128x256-conv", C2, "skip640", "reslo", (128, 256, 1, T3), (K_TILE, 128, 256, 1)),
    _c("tile128x320-conv", C2, "skip320", "plain", (128, 320, 1, T3), (K_TILE, 128, 320, 1)),
    _c("tile256x128-conv", C2, "n1280", "outlo", (256, 128, 1, T3), (K_TILE, 256, 128, 1)),
    # ---- kernel 1, the 4-phase 256-row kernel (epilogue_direct, Stat4)
    _c("phase256x256-dense", D2, "skip640", "plain", (256, 256, 1, 4), (K_PHASE, 256, 256, 1)),
    _c("phase256x320-dense", D2, "skip320", "reslo", (256, 320, 1, 4), (K_PHASE, 256, 320, 1)),
    _c("phase256x256-conv", C2, "h1280of1920", "emb", (256, 256, 1, 4), (K_PHASE, 256, 256, 1)),
    _c("phase256x320-conv", C2, "skip640", "outlo", (256, 320, 1, 4), (K_PHASE, 256, 320, 1)),
    # ---- kernel 2, the 2-stage dense tiles
    _c("shallow64x64", D2, "skip320", "reslo", (64, 64, 1, 2), (K_SHALLOW, 64, 64, 1)),
    _c("shallow64x128", D2K64, "skip640", "plain", (64, 128, 1, 2), (K_SHALLOW, 64, 128, 1)),
    # ---- kernel 3, the halo conv tiles
    _c("halo128-w16", C2, "n320", "emb", (256, 128, 1, 9), (K_HALO, 256, 128, 1), None,
       "ResBlock conv1 (the B = 1 / batched halo producer)"),
    _c("halo160-w16", C2, "skip640", "outlo", (256, 160, 1, 9), (K_HALO, 256, 160, 1)),
    _c("halo192-w16", C2, "n1280", "reslo", (256, 192, 1, 9), (K_HALO, 256, 192, 1)),
    _c("halo128-w16-split2", C2C128, "skip320", "plain", (256, 128, 2, 9), (K_HALO, 256, 128, 2), "reduce"),
    _c("halo64-w64", C2W64, "n320", "emb", (256, 64, 1, 9), (K_HALO, 256, 64, 1)),
    # ---- kernel 4, the deep ring; the BK = 32 rings (force_bm < 0)
    _c("deep4-64x64", D2, "skip320", "outlo", (64, 64, 1, 104), (K_DEEP, 64, 64, 1)),
    _c("deep4-64x64-conv", C2, "skip320", "reslo", (64, 64, 1, 104), (K_DEEP, 64, 64, 1)),
    _c("ring64x64-dense", D2, "h640of960", "plain", (-64, 64, 1, 0), (K_TILE, -64, 64, 1)),
    _c("ring64x64-conv", C2, "skip320", "outlo", (-64, 64, 1, 0), (K_TILE, -64, 64, 1)),
    _c("ring64x128-dense", D2, "skip640", "reslo", (-64, 128, 1, 0), (K_TILE, -64, 128, 1)),
    _c("ring64x128-conv", C2, "hi2560", "plain", (-64, 128, 1, 0), (K_TILE, -64, 128, 1)),
    _c("ring128x128-dense", D2, "skip320", "outlo", (-128, 128, 1, 0), (K_TILE, -128, 128, 1)),
    _c("ring128x128-conv", C2, "n320", "emb", (-128, 128, 1, 0), (K_TILE, -128, 128, 1)),
    _c("ring128x256-dense", D2, "skip640", "plain", (-128, 256, 1, 0), (K_TILE, -128, 256, 1)),
    _c("ring128x256-conv", C2, "skip640", "outlo", (-128, 256, 1, 0), (K_TILE, -128, 256, 1)),
    _c("ring128x320-dense", D2, "skip320", "plain", (-128, 320, 1, 0), (K_TILE, -128, 320, 1)),
    _c("ring128x320-conv", C2, "skip320", "reslo", (-128, 320, 1, 0), (K_TILE, -128, 320, 1)),
    _c("ring256x128-dense", D2, "n640", "emb", (-256, 128, 1, 0), (K_TILE, -256, 128, 1)),
    _c("ring256x128-conv", C2, "skip320", "outlo", (-256, 128, 1, 0), (K_TILE, -256, 128, 1)),
    _c("ring256x256-dense", D2, "skip640", "reslo", (-256, 256, 1, 0), (K_TILE, -256, 256, 1)),
    _c("ring256x256-conv", C2, "lo2560", "emb", (-256, 256, 1, 0), (K_TILE, -256, 256, 1)),
    # ---- kernel 0, the other built 256-row tiles
    _c("tile256x160-dense", D2, "skip320", "outlo", (256, 160, 1, T3), (K_TILE, 256, 160, 1)),
    _c("tile256x160-conv", C2, "skip640", "plain", (256, 160, 1, T3), (K_TILE, 256, 160, 1)),
    _c("tile256x256-dense", D2, "n1280", "emb", (256, 256, 1, T3), (K_TILE, 256, 256, 1)),
    _c("tile256x256-conv", C2, "skip640", "reslo", (256, 256, 1, T3), (K_TILE, 256, 256, 1)),
    _c("tile256x320-dense", D2, "skip640", "outlo", (256, 320, 1, T3), (K_TILE, 256, 320, 1)),
    _c("tile256x320-conv", C2, "skip320", "plain", (256, 320, 1, T3), (K_TILE, 256, 320, 1)),
    # ---- kernel 5, the two-K-group tiles: the two-target / offset geometry only
    _c("kgroup64x64-dense", D2, "skip320", "outlo", (64, 64, 1, 203), (K_KGROUP, 64, 64, 1)),
    _c("kgroup64x64-conv", C2, "skip320", "plain", (64, 64, 1, 203), (K_KGROUP, 64, 64, 1)),
    _c("kgroup64x128-dense", D2, "skip640", "outlo", (64, 128, 1, 203), (K_KGROUP, 64, 128, 1)),
    _c("kgroup64x128-conv", C2, "skip640", "reslo", (64, 128, 1, 203), (K_KGROUP, 64, 128, 1)),
    _c("kgroup64x128-conv-s2-coop", C2, "skip640", "outlo", (64, 128, 2, 203), (K_KGROUP, 64, 128, 2), "coop"),
    # ---- the other loader modes under the planner's own plan (tickets and workspace as the product passes them)
    _c("downsample", S2, "n320", "outlo", None, (K_TILE, 64, 64, 3), "coop", "Downsample conv"),
    _c("upsample", UP, "skip640", "outlo", None, (K_TILE, 64, 128, 3), "coop", "Upsample conv"),
    _c("input-conv", SMALLC, "skip320", "outlo", None, (K_TILE, 64, 128, 1), "coop", "input conv (4 channels)"),
    # ---- plan adjustments
    _c("hw64-128x128", DHW64, "skip320", "outlo", (128, 128, 1, T3), (K_TILE, 64, 128, 1)),
    _c("hw64-256x128", DHW64, "skip640", "reslo", (256, 128, 1, T3), (K_TILE, 64, 128, 1)),
    _c("hw64-128x320", DHW64, "n1280", "emb", (128, 320, 1, T3), (K_TILE, 64, 128, 1)),
    _c("hw64-ring128x320", DHW64, "hi2560", "plain", (-128, 320, 1, 0), (K_TILE, -64, 128, 1)),
    _c("hw320-phase256x320", DHW320, "skip320", "plain", (256, 320, 1, 4), (K_TILE, 64, 128, 1)),
    _c("m900-128x128", C900, "skip320", "outlo", (128, 128, 1, T3), (K_TILE, 64, 128, 1)),
    _c("m900-own", C900, "skip320", "emb", None, (K_KGROUP, 64, 128, 1), "coop",
       "ResBlock conv1 at B = 1 (two-K-group tiles)"),
    # ---- split-K: the reduce kernel on a 128-row tile
    _c("tile128x128-dense-s2-reduce", D2, "skip320", "plain", (128, 128, 2, T3), (K_TILE, 128, 128, 2), "reduce"),
]
# ---- split-K on the 64-row tiles under the three combines
for _bn, _geom, _epi in ((64, "skip320", "outlo"), (128, "skip640", "reslo")):
    for _s in (2, 3):
        for _mode in ("coop", "last", "reduce"):
            CASES.append(_c(f"tile64x{_bn}-dense-s{_s}-{_mode}", D2, _geom, _epi, (64, _bn, _s, T3),
                            (K_TILE, 64, _bn, _s), _mode))
CASES += [
    _c("tile64x64-conv-s3-coop", C2, "n320", "emb", (64, 64, 3, T3), (K_TILE, 64, 64, 3), "coop"),
    _c("tile64x128-conv-s2-last", C2, "skip640", "plain", (64, 128, 2, T3), (K_TILE, 64, 128, 2), "last"),
]
# the product's statistics producers: each must be named by the stands_for of a case (tests/test_gn_stats_cpu.py);
# the two concat norms are the CHAINS below
PRODUCERS = ("ResBlock conv1", "conv2 without the skip K-extension", "conv2 with the skip K-extension",
             "composite proj_out", "Downsample conv", "Upsample conv", "input conv")
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


# ---- operands and references ------------------------------------------------------------------------------
def pack_conv_w(w: torch.Tensor) -> torch.Tensor:
    """[N, C, 3, 3] -> [N][K] in the GEMM's K order (kernels.h AMode): channel-chunk-major
    k = (c / 64 * 9 + tap) * 64 + c % 64 when C % 64 == 0, else tap-major k = tap * C + c padded to 64."""
    n, c = w.shape[:2]
    p = w.permute(0, 2, 3, 1).reshape(n, 9, c)
    if c % 64 == 0:
        p = p.reshape(n, 9, c // 64, 64).permute(0, 2, 1, 3)
    p = p.reshape(n, 9 * c)
    K = (9 * c + 63) // 64 * 64
    out = torch.zeros(n, K, dtype=w.dtype)
    out[:, :9 * c] = p
    return out


def conv_ref(x: torch.Tensor, w: torch.Tensor, amode: int) -> torch.Tensor:
    """3x3 conv, pad 1, on NHWC x [B, H, W, C] with w [N, C, 3, 3] as nine shifted matrix products: stride 1,
    stride 2 (CONV3_S2, symmetric padding) or over the nearest-x2 upsampled input (CONV3_UP).  -> [B Ho Wo, N]."""
    if amode == A_CONV3_UP:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    s = 2 if amode == A_CONV3_S2 else 1
    B, H, W, C = x.shape
    Ho, Wo = H // s, W // s
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B * Ho * Wo, w.shape[0], dtype=x.dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            y += xp[:, ky:ky + s * Ho:s, kx:kx + s * Wo:s].reshape(-1, C) @ w[:, :, ky, kx].t()
    return y


class Ops:
    """The operands of (source, N, feature set) on a device and the fp64 reference [M, N] of the value the epilogue
    rounds (computed once, on that device, from the bf16 / fp32 operand values)."""

    def __init__(self, src, N, epi, dev):
        self.src, self.N, self.epi, self.dev = src, N, epi, dev
        self.B, self.hw, self.M = src_shape(src)
        f = EPI[epi]
        gen = torch.Generator().manual_seed(zlib.crc32(repr((src, N, epi)).encode()))
        B, hw, M = self.B, self.hw, self.M
        mu = torch.tensor(MU[:B])
        t: Dict[str, torch.Tensor] = {}
        if src[0] == "dense":
            K, Kx = src[3], src[4]
            self.amode, self.K, self.Kx = A_DENSE, K, Kx
            t["A"] = (torch.randn(B, hw, K, generator=gen) + mu.view(B, 1, 1)).reshape(M, K).to(torch.bfloat16)
            w = (torch.randn(N, K, generator=gen) / K ** 0.5 + 1.5 / K).to(torch.bfloat16)
            self.conv_w = None
        else:
            _, amode, _, H, W, C, Kx = src
            self.amode, self.H, self.W, self.C, self.Kx = amode, H, W, C, Kx
            t["A"] = (torch.randn(B, H, W, C, generator=gen) + mu.view(B, 1, 1, 1)).to(torch.bfloat16)
            self.conv_w = (torch.randn(N, C, 3, 3, generator=gen) / (9 * C) ** 0.5 + 1.5 / (9 * C)).to(torch.bfloat16)
            w = pack_conv_w(self.conv_w)
            self.K = w.shape[1]
        if self.Kx:
            t["X"] = (torch.randn(B, hw, self.Kx, generator=gen) - 0.5 * mu.view(B, 1, 1)).reshape(M, self.Kx).to(torch.bfloat16)
            wx = (torch.randn(N, self.Kx, generator=gen) / self.Kx ** 0.5).to(torch.bfloat16)
            w = torch.cat([w, wx], 1)
        t["Wt"] = w.contiguous()
        t["bias"] = torch.linspace(-1.5, 1.5, N) + 0.2 * torch.randn(N, generator=gen)  # a ramp over the channels
        if f.get("emb"):
            # B + 1 rows, batch element b reads row B - b: row 0 is never read
            shift = torch.tensor([7.0, 2.0, -1.0, 0.5, -2.0][:B + 1]).view(B + 1, 1)
            t["emb"] = torch.randn(B + 1, N + 4, generator=gen) * 0.5 + shift
            t["emb_row"] = torch.tensor([B - b for b in range(B)], dtype=torch.int32)
        if f.get("res"):
            r = torch.randn(M, N, generator=gen) * 1.5 + 0.3
            hi = r.to(torch.bfloat16)
            t["res"] = torch.stack([hi, (r - hi.float()).to(torch.bfloat16)]).contiguous()  # [2][M][N]
        self.act = f.get("act", 0)
        self.out_lo = bool(f.get("out_lo"))
        self.t = {k: v.to(dev) for k, v in t.items()}
        self._ref = None

    @property
    def ref(self) -> torch.Tensor:
        if self._ref is None:
            t = self.t
            w = t["Wt"].double()
            if self.amode == A_DENSE:
                y = t["A"].double() @ w[:, :self.K].t()
            else:
                y = conv_ref(t["A"].double(), self.conv_w.to(self.dev).double(), self.amode)
            if self.Kx:
                y = y + t["X"].double() @ w[:, self.K:].t()
            y = y + t["bias"].double()
            if "emb" in t:
                rows = t["emb"][t["emb_row"].long(), :self.N].double()  # [B, N]
                y = (y.view(self.B, self.hw, self.N) + rows[:, None, :]).reshape(self.M, self.N)
            if "res" in t:
                y = y + t["res"][0].double() + t["res"][1].double()
            if self.act == 1:
                y = y * torch.sigmoid(y)
            self._ref = y
        return self._ref

    def fields(self, ptr=None) -> Dict:
        """The descriptor fields of the operands; ptr: tensor -> pointer (default data_ptr; the CPU planning tests
        pass a constant)."""
        p = ptr or (lambda x: x.data_ptr())
        t = self.t
        f = dict(M=self.M, N=self.N, K=self.K, amode=self.amode, A=p(t["A"]), Wt=p(t["Wt"]), ldw=self.K + self.Kx,
                 bias=p(t["bias"]), rows_per_b=self.hw, act=self.act)
        if self.amode == A_DENSE:
            f.update(lda=self.K)
        else:
            s2, up = self.amode == A_CONV3_S2, self.amode == A_CONV3_UP
            Ho, Wo = (self.H // 2, self.W // 2) if s2 else (2 * self.H, 2 * self.W) if up else (self.H, self.W)
            f.update(lda=self.C, C=self.C, Bn=self.B, H=self.H, W=self.W, Ho=Ho, Wo=Wo)
        if self.Kx:
            f.update(X=p(t["X"]), ldx=self.Kx, Kx=self.Kx)
        if "emb" in t:
            f.update(emb=p(t["emb"]), ld_emb=t["emb"].shape[1], emb_row=p(t["emb_row"]))
        if "res" in t:
            f.update(res=p(t["res"]), ld_res=self.N, res_lo=self.M * self.N)
        return f


_OPS: Dict[tuple, Ops] = {}


def operands(case: Case, dev="cpu") -> Ops:
    key = (case.src, case.N, case.epi, str(dev))
    if key not in _OPS:
        _OPS[key] = Ops(case.src, case.N, case.epi, dev)
    return _OPS[key]


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


def stat_fields(targets: List[Tgt], ptrs, rs: List[int], hw: int) -> Dict:
    """st_* (and st2_*) of one or two targets at the accumulators ptrs with replica strides rs."""
    t = targets[0]
    f = dict(st_acc=ptrs[0], st_rs=rs[0], st_cg=t.cg, st_G=t.G, st_coff=t.c_off, st_hw=hw)
    if len(targets) > 1:
        t = targets[1]
        f.update(st2_acc=ptrs[1], st2_rs=rs[1], st2_cg=t.cg, st2_G=t.G, st2_coff=t.c_off)
    return f


PART_CAP = 1 << 23  # split-K workspace of the tests (fp32 elements)
SEM_CAP = 1 << 14


def combine_fields(mode: Optional[str], part_ptr, sem_ptr) -> Dict:
    """coop: tickets (the grid is resident: cooperative combine); last: tickets + probe bit 2 (last-arriver combine);
    reduce: no tickets (fp32 slabs summed by the reduce kernel)."""
    if mode is None:
        return {}
    kw = dict(partial=part_ptr, partial_cap=PART_CAP)
    if mode in ("coop", "last"):
        kw.update(tile_sem=sem_ptr, sem_cap=SEM_CAP)
    if mode == "last":
        kw.update(probe=4)
    return kw


def plan_of(d) -> Tuple[int, Tuple[int, int, int, int]]:
    """(status, (kernel, bm, bn, splits)) of tair_k_gemm_plan: host only."""
    from tair_amd import _lib
    o = [ctypes.c_int() for _ in range(4)]
    rc = _lib.lib().tair_k_gemm_plan(ctypes.byref(d), *[ctypes.byref(x) for x in o])
    bm, bn, splits, kern = (x.value for x in o)
    return rc, (kern, bm, bn, splits)


def planning_desc(case: Case):
    """The case's descriptor with placeholder pointers: what tair_k_gemm_plan needs (no device, no operands)."""
    B, hw, M = src_shape(case.src)
    o = operands(case, "cpu")
    n = len(case.targets)
    return make_desc(out=64, ldo=case.N + 24, **o.fields(lambda x: 64), **force_fields(case.force),
                     **stat_fields(case.targets, [64] * n, [2 * B * G] * n, hw), **combine_fields(case.combine, 64, 64),
                     **(dict(out_lo=(M + 8) * (case.N + 24)) if case.hilo else {}))


# ---- statistics references ---------------------------------------------------------------------------------
def slot_sums(v: torch.Tensor, B: int, hw: int, t: Tgt):
    """fp64 [B, G] (sum v, sum v^2, sum |v|, number of values) per (batch element, group) of target t over the
    stored values v [B * hw, N]: channel n belongs to group (c_off + n) // cg."""
    N = v.shape[1]
    v = v.double().view(B, hw, N)
    gi = (t.c_off + torch.arange(N, device=v.device)) // t.cg
    keep = gi < t.G
    cols = torch.stack([v.sum(1), (v * v).sum(1), v.abs().sum(1), torch.full((B, N), float(hw), dtype=torch.float64,
                                                                               device=v.device)])
    out = torch.zeros(4, B, t.G, dtype=torch.float64, device=v.device)
    out.index_add_(2, gi[keep], cols[:, :, keep])
    return out[0], out[1], out[2], out[3]


def slot_errors(got: torch.Tensor, sums, hilo: bool):
    """got [B, G, 2] against (s, q, sa, cnt) of slot_sums (added up over the producers of a shared slot): the worst
    |deviation| / bound over the owned slots, for the sums and for the sums of squares.
    plain bf16 output (the kernel adds the stored values in fp64, in any order; the factor 2 covers the eight
    replicas the test adds up):   |S - got| <= 2 n 2^-53 sum|v|,  |Q - got| <= 2 n 2^-53 sum v^2
    hi + lo output (the kernel adds the fp32 value v, stored to 2^-16 |v|; tests/test_ffpout_gpu.py _check_stats):
                                  |S - got| <= 2^-16 sum|v|,     |Q - got| <= (2^-15 + 2^-32) sum v^2"""
    s, q, sa, cnt = sums
    own = cnt > 0
    if hilo:
        bs, bq = 2.0 ** -16 * sa, (2.0 ** -15 + 2.0 ** -32) * q
    else:
        bs, bq = 2 * cnt * 2.0 ** -53 * sa, 2 * cnt * 2.0 ** -53 * q
    es = ((got[..., 0] - s).abs()[own] / bs[own]).max().item()
    eq = ((got[..., 1] - q).abs()[own] / bq[own]).max().item()
    return es, eq, own


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bf16_floor(ref):
    return rel_l2(ref.to(torch.bfloat16), ref)


# ---- the concat GroupNorm ------------------------------------------------------------------------------------
# (channels of h, its forced plan; channels of the skip, its forced plan): cat([h, skip]) in 32 groups
CHAINS = {
    960: (("h640of960", (64, 64, 1, T3)), ("skip320", (128, 128, 1, T3))),     # cg 30, group 21 shared
    1920: (("h1280of1920", (128, 256, 1, T3)), ("skip640", (64, 128, 1, T3))),  # cg 60, group 21 shared
}
GN_EPS = 1e-5


def chain_cases(C: int):
    (gh, fh), (gs, fs) = CHAINS[C]
    return (Case(f"chain{C}-h", D2, gh, "plain", fh, (K_TILE,) + fh[:3]),
            Case(f"chain{C}-skip", D2K64, gs, "plain", fs, (K_TILE,) + fs[:3]))


def gn_params(C: int, dev="cpu"):
    gen = torch.Generator().manual_seed(C)
    return (torch.rand(C, generator=gen) + 0.5).to(dev), torch.randn(C, generator=gen).to(dev)


def gn_ref(x: torch.Tensor, B: int, hw: int, gamma, beta) -> torch.Tensor:
    """fp64 F.group_norm (G groups, eps GN_EPS) of the stored NHWC tensor x [B * hw, C] -> [B * hw, C]."""
    C = x.shape[1]
    y = F.group_norm(x.double().view(B, hw, C).permute(0, 2, 1), G, gamma.double(), beta.double(), GN_EPS)
    return y.permute(0, 2, 1).reshape(B * hw, C)


def gn_emulate(x: torch.Tensor, B: int, hw: int, gamma, beta) -> torch.Tensor:
    """The apply's arithmetic with exact statistics: mean and rstd from fp64 sums rounded to fp32, an fp32 affine
    x * (gamma rstd) + (beta - mean gamma rstd), one bf16 rounding."""
    C = x.shape[1]
    cg = C // G
    v = x.double().view(B, hw, G, cg)
    cnt = float(hw * cg)
    mean = v.sum((1, 3)) / cnt
    var = ((v * v).sum((1, 3)) / cnt - mean * mean).clamp_min(0)
    mean32 = mean.float().repeat_interleave(cg, 1)          # [B, C]
    rstd32 = (1.0 / torch.sqrt(var + GN_EPS)).float().repeat_interleave(cg, 1)
    sc = gamma.float() * rstd32
    sh = beta.float() - mean32 * sc
    y = x.float().view(B, hw, C) * sc[:, None, :] + sh[:, None, :]
    return y.to(torch.bfloat16).reshape(B * hw, C)


def block_ratios(got: torch.Tensor, ref: torch.Tensor, B: int, hw: int) -> torch.Tensor:
    """[B, G]: rel-L2 of got against ref over each (batch element, group) block / that block's bf16 rounding floor."""
    C = ref.shape[1]
    r = ref.double().view(B, hw, G, C // G)
    g = got.double().view(B, hw, G, C // G)
    fl = (r.to(torch.bfloat16).double() - r).pow(2).sum((1, 3)).sqrt()
    return (g - r).pow(2).sum((1, 3)).sqrt() / fl
