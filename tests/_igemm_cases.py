"""Cases, float64 oracle, derived bounds, dispatch mirror and seeded faults for the implicit GEMM (csrc/igemm.hip: st_conv,
st_conv_batch).  CPU only (numpy / torch float64); tests/test_igemm_inputs.py shows that the bounds hold for a float32 / bf16
replica of the oracle and that every seeded fault breaks them, tests/test_gpu_igemm.py runs the kernel against them.

  y[m][n] = sum_k x_gather[m][k] * w[n][k]     m = (b, ho, wo), k = (kh, kw, c)
  v = acc + bias;  stats += [sum v | sum v*v];  v = v * scale + shift;  v += residual;  v = max(v, 0);  y = (accumulate ? y : 0) + v

Inputs.  Seeded, rounded to the case's storage type (so the float64 oracle and the kernel read the same numbers), drawn with a
non-zero mean so that no result is a sum that cancels to nothing, and different in every row and column (test_igemm_inputs.py
checks it).  Every buffer has its leading dimension: pad columns of x, w and the residual hold NaN, pad columns of y, a guard row
after row M - 1 and (with `y_off`) the 16 bytes in front of the base pointer hold a canary pattern.

Bounds, u = 2^-24.  T[m][n] is the sum of the absolute values of every term that enters the element:
  T = |scale| * (sum_k |x w| + |bias|) + |shift| + |residual| + |y_old|
  |got - ref| <= c * (K + 8) * u * T                      an fp32 fma chain of K terms in any order, and at most 8 further roundings
                 (* (1 + 2^-8) + 2^-8 |ref| for bf16 output: 8 significand bits, round to nearest)
  + E             input transform only: what the fp32 BatchNorm coefficients and (bf16) the rounding of relu(bn(x)) to the
                  operand type can move the element by, see `_transform`
Statistics (per channel, M rows):  with Tv = sum_k |x w| + |bias| per row,
  |sum  - ref| <= c * ((K + 8) + (M + 8)) * u * sum_m Tv
  |sumsq - ref| <= c * (2 (K + 8) + 1 + (M + 8)) * u * sum_m Tv^2      (v^2: twice the relative error of v, one rounding)
c = C_BOUND[dtype]: 1 for fp32 operands (the fp32 MFMA is a k-ordered fma chain); for bf16 operands the products are exact in
fp32 and the measured error on an MI355X decides (DESIGN.md section 7, row 'implicit GEMM').
"""
import functools
import zlib

import numpy as np
import torch

DTYPES = ("float32", "bfloat16")
TORCH_DTYPE = {"float32": torch.float32, "bfloat16": torch.bfloat16}
CODE = {"float32": 0, "bfloat16": 1}          # ST_F32, ST_BF16
EPC = {"float32": 4, "bfloat16": 8}           # elements per 16-byte chunk
U = 2.0 ** -24
UB = 2.0 ** -8                                # unit roundoff of bf16
C_BOUND = {"float32": 1.0, "bfloat16": 1.0}
GROUP = 12                                    # kGroup: members of one launch
KNOBS = (0, 0, 1)                             # st_tune(ring, kc, w8) defaults
EPS = 1e-5
ROUTE_FIELDS = ("loop", "BM", "BN", "waves", "KC", "MODE", "members", "atomic")

_DEFAULT = dict(B=1, Hin=1, Win=1, Cin=0, N=0, KH=1, KW=1, stride=1, pad=0, ldx=None, ldx_pad=0, ldw_pad=0, ldy_pad=0, y_off=False,
                bias=False, stats=False, srep=0, affine=False, residual=False, relu=False, accumulate=False, out=None, k_order=0,
                split_k=0, xf=False, group=1, knobs=KNOBS, dtypes=DTYPES)


def gemm(M, N, K, route, why, **opt):
    return dict(_DEFAULT, B=M, Cin=K, N=N, route=route, why=why, **opt)


def conv(B, Hin, Win, Cin, N, KH, KW, stride, pad, route, why, **opt):
    return dict(_DEFAULT, B=B, Hin=Hin, Win=Win, Cin=Cin, N=N, KH=KH, KW=KW, stride=stride, pad=pad, route=route, why=why, **opt)


# route: (main loop, BM, BN, waves, KC, MODE); MODE as (fp32, bf16) where the two differ (a K tile is 32 fp32 / 64 bf16 elements)
R_128x64 = (0, 128, 64, 8, 8)
R_128x64_4W = (0, 128, 64, 4, 8)
R_64x128 = (0, 64, 128, 4, 8)
R_128 = (0, 128, 128, 8, 8)
R_128_4W = (0, 128, 128, 4, 8)
R_256 = (0, 256, 128, 8, 8)
R_S3B = (2, 128, 128, 4, 4, 1)
FULL = dict(bias=True, stats=True, affine=True, residual=True, relu=True, accumulate=True)

CASES = {
    # ---- GEMM form: one case per tile and K-chunk route ------------------------------------------------------------------
    "g128x64_fast": gemm(129, 60, 64, R_128x64 + (1,), "128x64, whole K tiles (MODE 1)"),
    "g128x64_walk": gemm(129, 60, 72, R_128x64 + (0,), "128x64, generic tap walk (MODE 0): K is no multiple of a tile"),
    "g_m_le_64": gemm(5, 132, 64, R_64x128 + (1,), "64x128 through M <= 64"),
    "mid": gemm(300, 200, 136, R_128 + (0,), "128x128 below both tile-count thresholds"),
    "g_t64": gemm(1100, 1800, 32, R_64x128 + ((1, 0),), "64x128 through t64 >= 256"),
    "g_t128": gemm(3000, 2052, 32, R_128 + ((1, 0),), "128x128 through t128 >= 384"),
    "kc4_128x64": gemm(4100, 60, 128, (0, 128, 64, 4, 4, 1), "KC 4 (short K, M >= 4096) on 128x64, 4 waves"),
    "kc4_128": gemm(4100, 200, 64, (0, 128, 128, 8, 4, 1), "KC 4 on 128x128"),
    "kc4_64x128": gemm(4100, 600, 64, (0, 64, 128, 4, 4, 1), "KC 4 on 64x128"),
    "three_buffer": gemm(2050, 1990, 1024, R_S3B, "the default three-buffer DMA route: bf16, K >= 1024, Cin >= 256, >= 256 tiles",
                         dtypes=("bfloat16",), ldy_pad=2),       # ldy must be a multiple of 4
    # ---- leading dimensions and a base pointer that is only 16-byte aligned ------------------------------------------------
    "mid_ld4": gemm(300, 200, 136, R_128 + (0,), "ldx = K + 8, ldw = K + 16, ldy = N + 4: element-wise stores",
                    ldx_pad=8, ldw_pad=16, ldy_pad=4, y_off=True),
    "mid_ld8": gemm(300, 200, 136, R_128 + (0,), "ldy = N + 8: vector stores beside pad columns", ldx_pad=8, ldw_pad=16, ldy_pad=8, y_off=True),
    "g128x64_ld4": gemm(129, 60, 64, R_128x64 + (1,), "128x64 with every leading dimension padded, ldy % 8 != 0",
                        ldx_pad=8, ldw_pad=16, ldy_pad=4, y_off=True),
    "g128x64_ld8": gemm(129, 60, 64, R_128x64 + (1,), "128x64, ldy = N + 8 (N % 8 = 4: the last chunk is a tail)",
                        ldx_pad=8, ldw_pad=16, ldy_pad=8, y_off=True),
    # ---- convolutions ------------------------------------------------------------------------------------------------
    "c3_small": conv(1, 9, 11, 16, 24, 3, 3, 1, 1, R_128x64 + (0,), "3x3 with Cin below a K tile: per-thread tap walk"),
    "c3_s2": conv(2, 15, 17, 64, 68, 3, 3, 2, 1, R_128 + (1,), "3x3 stride 2, odd map, whole-tile taps with a padding mask"),
    "c3_s2_ko1": conv(2, 15, 17, 64, 68, 3, 3, 2, 1, R_128 + (1,), "the same with chunk-major weights (k_order 1)", k_order=1),
    "c3_ko1_c128": conv(2, 15, 17, 128, 68, 3, 3, 2, 1, R_128 + (1,), "k_order 1 over more than one 128-byte chunk of channels", k_order=1),
    "stem": conv(2, 33, 35, 8, 64, 7, 7, 2, 3, R_128x64 + (0,), "the stem geometry: 7x7 s2 p3, Cin 8"),
    "taps64": conv(1, 12, 12, 64, 24, 8, 8, 1, 4, R_128x64 + (1,), "64 taps: the limit of MODE 1's tap mask"),
    "taps81": conv(1, 12, 12, 64, 24, 9, 9, 1, 4, R_128x64 + (0,), "81 taps: past the mask, MODE 0"),
    "k3x1": conv(2, 9, 7, 32, 40, 3, 1, 1, 0, R_128x64 + ((1, 0),), "KH 3, KW 1, no padding"),
    "sliding": conv(2, 12, 13, 64, 64, 4, 1, 2, 0, R_128x64 + (1,), "sliding window: ldx 16 < Cin 64, four pixels per tap", ldx=16),
    # ---- input transform (MODE 2) ------------------------------------------------------------------------------------
    "xf_k1": conv(2, 9, 11, 64, 72, 1, 1, 1, 0, R_128 + (2,), "relu(bn(x)) in the loader, 1x1, ragged M", xf=True),
    "xf_k3": conv(2, 9, 11, 128, 72, 3, 3, 1, 1, R_128 + (2,), "relu(bn(x)) in the loader, 3x3: padding taps stay zero", xf=True),
    "xf_k3_s2": conv(3, 9, 11, 64, 40, 3, 3, 2, 1, R_128x64 + (2,), "relu(bn(x)) in the loader, 3x3 stride 2, 128x64", xf=True),
    # ---- epilogue: each option alone, then the whole chain; N = 132 leaves a tail chunk ----------------------------------
    "e_bias": gemm(150, 132, 72, R_128 + (0,), "bias alone", bias=True),
    "e_stats": gemm(150, 132, 72, R_128 + (0,), "statistics alone", stats=True),
    "e_stats_bias": gemm(150, 132, 72, R_128 + (0,), "statistics of acc + bias", stats=True, bias=True),
    "e_affine": gemm(150, 132, 72, R_128 + (0,), "scale / shift alone", affine=True),
    "e_residual": gemm(150, 132, 72, R_128 + (0,), "residual alone", residual=True),
    "e_relu": gemm(150, 132, 72, R_128 + (0,), "relu alone", relu=True),
    "e_accumulate": gemm(150, 132, 72, R_128 + (0,), "accumulate alone", accumulate=True),
    "e_full": gemm(300, 132, 72, R_128 + (0,), "bias -> stats -> scale/shift -> residual -> relu -> accumulate, three pixel tiles", **FULL),
    "e_full_f32out": gemm(300, 132, 72, R_128 + (0,), "the whole chain into fp32 output", out="float32", **FULL),
    "e_full_ld4": gemm(300, 132, 72, R_128 + (0,), "the whole chain through the element-wise stores", ldy_pad=4, y_off=True, **FULL),
    "e_full_rep3": gemm(500, 132, 72, R_128 + (0,), "three statistics replicas over four pixel tiles", srep=3, **FULL),
    "e_full_rep3_64": gemm(530, 60, 64, R_128x64 + (1,), "three statistics replicas over five 128x64 pixel tiles",
                           srep=3, **FULL),
    "e_stats_small": gemm(33, 60, 64, R_128x64 + (1,), "statistics of few rows: rounding y before them would show", stats=True, bias=True,
                          relu=True),
    # ---- split-K: fp32 output, slices as members of one launch, atomics ---------------------------------------------------
    "sk2": gemm(77, 100, 256, R_128 + (1,), "split-K 2", split_k=2, out="float32", bias=True),
    "sk12": gemm(77, 100, 1536, R_128 + (1,), "split-K 12", split_k=12, out="float32", bias=True),
    "sk2_acc": gemm(300, 132, 256, R_128 + (1,), "split-K 2 onto an old y", split_k=2, out="float32", bias=True, accumulate=True),
    "sk12_acc": gemm(300, 132, 1536, R_128 + (1,), "split-K 12 onto an old y", split_k=12, out="float32", bias=True, accumulate=True),
    "sk2_300": gemm(300, 132, 256, R_128 + (1,), "split-K 2 over three pixel tiles", split_k=2, out="float32", bias=True),
    "sk2_acc77": gemm(77, 100, 256, R_128 + (1,), "split-K 2 onto an old y, one tile", split_k=2, out="float32", bias=True, accumulate=True),
    "sk12_acc77": gemm(77, 100, 1536, R_128 + (1,), "split-K 12 onto an old y, one tile", split_k=12, out="float32", bias=True, accumulate=True),
    "sk2_ld4": gemm(77, 100, 256, R_128 + (1,), "split-K 2 with pad columns: the zero fill must leave them alone", split_k=2, out="float32",
                    bias=True, ldy_pad=4, y_off=True),
    "sk12_ld4": gemm(300, 132, 1536, R_128 + (1,), "split-K 12 with pad columns", split_k=12, out="float32", bias=True, ldy_pad=4, y_off=True),
    # ---- grouped launch -------------------------------------------------------------------------------------------------
    "grp1": gemm(150, 132, 72, R_128 + (0,), "st_conv_batch with one member", group=1, bias=True, accumulate=True, out="float32"),
    "grp12": gemm(150, 132, 72, R_128 + (0,), "st_conv_batch with twelve members", group=12, bias=True, accumulate=True, out="float32"),
    # ---- routes only the knobs reach (st_tune) --------------------------------------------------------------------------
    "w8_0_mid": gemm(300, 200, 136, R_128_4W + (0,), "w8 = 0: 128x128 as 2x2 waves", knobs=(0, 0, 0)),
    "w8_0_c3": conv(1, 9, 11, 16, 24, 3, 3, 1, 1, R_128x64_4W + (0,), "w8 = 0: 128x64 with 4 waves", knobs=(0, 0, 0)),
    "w8_2_gemm": gemm(16400, 132, 32, R_256 + ((1, 0),), "w8 = 2: 256x128", knobs=(0, 0, 2)),
    "w8_2_c3": conv(2, 96, 96, 8, 72, 3, 3, 1, 1, R_256 + (0,), "w8 = 2: 256x128 on a 3x3", knobs=(0, 0, 2)),
    "kc4_mid": gemm(300, 200, 136, (0, 128, 128, 8, 4, 0), "kc = 4 forced on a long ragged K", knobs=(0, 4, 1)),
    "kc4_c3": conv(1, 9, 11, 16, 24, 3, 3, 1, 1, (0, 128, 64, 4, 4, (1, 0)), "kc = 4 forced on a 3x3", knobs=(0, 4, 1)),
    "ring4_gemm": gemm(300, 200, 192, R_S3B, "ring 4: the three-buffer route at a small shape", knobs=(4, 0, 1), dtypes=("bfloat16",)),
    "ring4_c3": conv(2, 15, 17, 64, 68, 3, 3, 2, 1, R_S3B, "ring 4 on a 3x3 with padding taps", knobs=(4, 0, 1), dtypes=("bfloat16",)),
    "ring4_c3_ko1": conv(2, 15, 17, 128, 68, 3, 3, 2, 1, R_S3B, "ring 4 with chunk-major weights", knobs=(4, 0, 1), k_order=1,
                         dtypes=("bfloat16",)),
}
# tails: K one and a half tiles (the second K tile is half empty), one launch per pair on the diagonal of the grid
TAIL_M = (1, 63, 64, 65, 127, 128, 129)
TAIL_N = (4, 60, 64, 68, 124, 128, 132)
for _m, _n in zip(TAIL_M, TAIL_N):
    for _dt in DTYPES:
        _k = 48 if _dt == "float32" else 96
        CASES[f"tail_{_m}x{_n}_{_dt[0]}"] = gemm(_m, _n, _k, ((R_128x64 if _n <= 64 else R_64x128 if _m <= 64 else R_128) + (0,)),
                                                 f"ragged edges M = {_m}, N = {_n}", dtypes=(_dt,), bias=True)

RUNS = [(name, dt) for name, s in CASES.items() for dt in s["dtypes"]]


# ---- geometry, descriptor, route -----------------------------------------------------------------------------------------

def geometry(s):
    sliding = s["ldx"] is not None and s["ldx"] < s["Cin"]
    if sliding:
        Ho, Wo = (s["Hin"] - s["KH"]) // s["stride"] + 1, (s["Win"] - s["Cin"] // s["ldx"]) // s["stride"] + 1
    else:
        Ho, Wo = (s["Hin"] + 2 * s["pad"] - s["KH"]) // s["stride"] + 1, (s["Win"] + 2 * s["pad"] - s["KW"]) // s["stride"] + 1
    K = s["KH"] * s["KW"] * s["Cin"]
    return dict(M=s["B"] * Ho * Wo, N=s["N"], K=K, Ho=Ho, Wo=Wo, ldx=s["ldx"] if s["ldx"] is not None else s["Cin"] + s["ldx_pad"],
                ldw=K + s["ldw_pad"], ldy=s["N"] + s["ldy_pad"], sliding=sliding)


def out_dtype(s, dtype):
    return s["out"] or dtype


def descriptor(s, dtype):
    """The integer fields of st_conv_desc and which optional pointers are given, as the GPU file passes them."""
    g = geometry(s)
    return dict(dtype=CODE[dtype], out_dtype=CODE[out_dtype(s, dtype)], B=s["B"], Hin=s["Hin"], Win=s["Win"], Cin=s["Cin"], Ho=g["Ho"],
                Wo=g["Wo"], N=s["N"], KH=s["KH"], KW=s["KW"], stride=s["stride"], pad=s["pad"], ldx=g["ldx"], ldw=g["ldw"], ldy=g["ldy"],
                relu=int(s["relu"]), accumulate=int(s["accumulate"]), Cin_logical=0, k_order=s["k_order"], stats_replicas=s["srep"],
                in_count=float(s["B"] * s["Hin"] * s["Win"]) if s["xf"] else 0.0, in_eps=EPS if s["xf"] else 0.0, split_k=s["split_k"],
                x=True, w=True, y=True, bias=s["bias"], scale=s["affine"], shift=s["affine"], residual=s["residual"], stats=s["stats"],
                in_stats=s["xf"], in_gamma=s["xf"], in_beta=s["xf"])


def desc_errors(d):
    """Mirror of fill_args' and st_conv's (split-K) ST_CHECKs: the messages of the requirements `d` violates, in their order."""
    errs = []
    bad = lambda cond, msg: errs.append(msg) if cond else None
    bad(not (d["x"] and d["w"] and d["y"]), "null pointer")
    bad(d["dtype"] not in (0, 1), "bad dtype")
    epc = 8 if d["dtype"] == 1 else 4
    bad(not (d["Cin"] > 0 and d["Cin"] % epc == 0), "Cin=")
    bad(d["ldx"] % epc or d["ldw"] % epc, "must be multiples of")
    sliding = d["ldx"] < d["Cin"]
    bad(sliding and not (d["KW"] == 1 and d["pad"] == 0 and d["ldx"] > 0 and d["Cin"] % d["ldx"] == 0 and not d["k_order"]
                         and (d["Wo"] - 1) * d["stride"] + d["Cin"] // max(d["ldx"], 1) <= d["Win"]
                         and (d["Ho"] - 1) * d["stride"] + d["KH"] <= d["Hin"]), "sliding-window input needs")
    bad(d["ldw"] < d["KH"] * d["KW"] * d["Cin"], "leading dimensions too small")
    bad(not 0 <= d["stats_replicas"] <= 1024, "bad stats_replicas")
    bad(d["ldy"] % 4 or d["ldy"] < d["N"], "ldy=")
    bad(not all(d[k] > 0 for k in ("B", "N", "Ho", "Wo", "KH", "KW", "stride")), "bad geometry")
    bad(d["Hin"] >= 32768 or d["Win"] >= 32768, "spatial size too large")
    bad(d["B"] * d["Hin"] * d["Win"] * d["ldx"] >= 1 << 40, "input too large")
    bad(bool(d["scale"]) != bool(d["shift"]), "scale and shift must be given together")
    bad(d["k_order"] and not (d["Cin"] % (8 * epc) == 0 and d["KH"] * d["KW"] <= 64), "k_order=1 needs")
    bad(d["in_stats"] and not (d["in_gamma"] and d["in_beta"] and d["in_count"] > 0 and d["ldx"] >= d["Cin"] and d["Cin"] <= 8192),
        "input transform needs gamma, beta, count")
    if d["split_k"] > 1:
        S, bk = d["split_k"], 64 if d["dtype"] == 1 else 32
        bad(not (S <= GROUP and d["KH"] == d["KW"] == d["Hin"] == d["Win"] == 1 and d["out_dtype"] == 0 and not d["relu"] and not d["scale"]
                 and not d["residual"] and not d["stats"] and not d["in_stats"] and d["Cin"] % (S * bk) == 0), f"split_k={S} needs")
    elif d["in_stats"] and not errs:      # `launch`, after dispatch; a K tile is 8 chunks unless the short-K rule applies (K % 64 == 0 there)
        bad(d["Cin"] % (8 * epc), "the input transform needs Cin to be a multiple")
    return errs


def route(s, dtype, knobs=None):
    """Mirror of dispatch / dispatch_kc / launch (csrc/igemm.hip): what st_conv_last_route reports for the case."""
    ring, kc, w8 = s["knobs"] if knobs is None else knobs
    g = geometry(s)
    S = max(s["split_k"], 1)
    M, N, Cin = g["M"], g["N"], s["Cin"] // S
    K, taps, bf16 = g["K"] // S, s["KH"] * s["KW"], dtype == "bfloat16"
    members, atomic = (S if S > 1 else s["group"]), int(S > 1)
    up = lambda a, b: (a + b - 1) // b
    t128 = up(M, 128) * up(N, 128)
    legal = bf16 and Cin % 64 == 0 and K % 64 == 0 and taps <= 64 and not s["xf"] and N > 64 and g["ldx"] >= Cin
    big3 = taps > 1 and Cin >= 256 and t128 >= 256
    if legal and (ring == 1 or (ring == 3 and big3)):
        return (1, 128, 128, 4, 8, 1, members, atomic)
    if legal and K >= 128 and ring != 2 and (ring == 4 or (ring == 5 and big3) or (ring == 0 and K >= 1024 and Cin >= 256 and t128 >= 256)):
        return (2, 128, 128, 4, 4, 1, members, atomic)
    short_k = taps == 1 and K <= 256 and K % 64 == 0 and M >= 4096
    KC = 4 if (kc == 4 or (kc == 0 and short_k)) and not s["k_order"] else 8
    if N <= 64:
        tile = (128, 64, 8) if KC == 8 and w8 and w8 != 3 else (128, 64, 4)
    elif w8 == 2 and M >= 256 * 64:
        tile = (256, 128, 8)
    elif t128 >= 384:
        tile = (128, 128, 8 if w8 else 4)
    elif up(M, 64) * up(N, 128) >= 256 or M <= 64:
        tile = (64, 128, 4)
    else:
        tile = (128, 128, 8 if w8 else 4)
    fast = Cin % (KC * EPC[dtype]) == 0 and taps <= 64
    assert fast or not s["xf"], "the input transform needs whole K tiles"
    return (0,) + tile + (KC, 2 if s["xf"] else int(fast), members, atomic)


def table_route(s, dtype):
    """The route the case table names for the case."""
    r = s["route"]
    mode = r[5][DTYPES.index(dtype)] if isinstance(r[5], tuple) else r[5]
    S = max(s["split_k"], 1)
    return r[:5] + (mode, S if S > 1 else s["group"], int(S > 1))


# ---- inputs -------------------------------------------------------------------------------------------------------------

def _round(a, dtype):
    """float64 array -> the nearest values of the storage type, as float64."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(TORCH_DTYPE[dtype]).double().numpy()


def canary(n, start=0):
    """The pattern untouched output memory holds: -100 .. -128 by position, exact in bf16 and far from every result."""
    return -(100.0 + ((np.arange(n) + start) % 29))


def korder_pack(w, s, dtype):
    """[N][KH][KW][Cin] -> [N][Cin/CH][KH][KW][CH], CH = 128 bytes of channels (k_order 1)."""
    CH = 8 * EPC[dtype]
    N = w.shape[0]
    return w.reshape(N, s["KH"], s["KW"], s["Cin"] // CH, CH).transpose(0, 3, 1, 2, 4).reshape(N, -1)


@functools.lru_cache(maxsize=6)
def inputs(name, dtype, member=0):
    """Everything one launch reads, as float64 arrays holding values of their storage types.  Flat buffers carry their pads."""
    s, g = CASES[name], geometry(CASES[name])
    M, N, K, ldx, ldw, ldy = g["M"], g["N"], g["K"], g["ldx"], g["ldw"], g["ldy"]
    odt = out_dtype(s, dtype)
    rng = np.random.default_rng(zlib.crc32(f"{name}/{dtype}/{member}".encode()))
    npix = s["B"] * s["Hin"] * s["Win"]
    x = np.full((npix, ldx), np.nan)
    cx = min(ldx, s["Cin"])
    x[:, :cx] = _round(rng.normal(0.25, 1.0, (npix, cx)), dtype)
    wl = _round(rng.normal(0.125, 1.0, (N, K)) / np.sqrt(K / 8.0), dtype)          # logical [N][KH][KW][Cin]
    w = np.full((N, ldw), np.nan)
    w[:, :K] = korder_pack(wl, s, dtype) if s["k_order"] else wl
    p = dict(x=x.reshape(-1), w=w, wl=wl)
    f32 = lambda a: _round(a, "float32")
    p["bias"] = f32(rng.normal(0.5, 1.0, N)) if s["bias"] else None
    p["scale"] = f32(rng.normal(0.0, 1.0, N) + np.where(np.arange(N) % 2, 1.5, -1.5)) if s["affine"] else None
    p["shift"] = f32(rng.normal(0.0, 1.0, N)) if s["affine"] else None
    if s["residual"]:
        r = np.full((M, ldy), np.nan)
        r[:, :N] = _round(rng.normal(0.0, 2.0, (M, N)), odt)
        p["residual"] = r
    else:
        p["residual"] = None
    lead = (16 // (2 if odt == "bfloat16" else 4)) if s["y_off"] else 0
    y0 = canary(lead + (M + 1) * ldy)
    if s["accumulate"]:
        body = y0[lead:].reshape(M + 1, ldy)
        body[:M, :N] = _round(rng.normal(0.0, 2.0, (M, N)), odt)
    p["y0"], p["lead"] = y0, lead
    R = max(s["srep"], 1)
    p["stats0"] = f32(rng.normal(0.0, 4.0, (R, 2 * N))) if s["stats"] else None
    if s["xf"]:     # the producer's batch statistics of x itself, its BatchNorm's weight and bias
        xs = x[:, :s["Cin"]]
        p["in_stats"] = f32(np.concatenate([xs.sum(0), (xs * xs).sum(0)]))
        p["in_gamma"] = f32(rng.normal(1.0, 0.25, s["Cin"]))
        p["in_beta"] = f32(rng.normal(0.1, 0.5, s["Cin"]))
    return p


# ---- oracle -------------------------------------------------------------------------------------------------------------

def _gather_index(s, g, ldx=None, clamp=False):
    """addr[m][k] into the flat x buffer and valid[m][k] (False: a padding tap, which contributes zero)."""
    ldx = g["ldx"] if ldx is None else ldx
    m = np.arange(g["M"])
    b, rem = m // (g["Ho"] * g["Wo"]), m % (g["Ho"] * g["Wo"])
    hi0, wi0 = (rem // g["Wo"]) * s["stride"] - s["pad"], (rem % g["Wo"]) * s["stride"] - s["pad"]
    k = np.arange(g["K"])
    kh, kw, c = k // (s["KW"] * s["Cin"]), (k // s["Cin"]) % s["KW"], k % s["Cin"]
    hi, wi = hi0[:, None] + kh[None, :], wi0[:, None] + kw[None, :]
    valid = (hi >= 0) & (hi < s["Hin"]) & (wi >= 0) & (wi < s["Win"])
    if clamp:
        hi, wi = np.clip(hi, 0, s["Hin"] - 1), np.clip(wi, 0, s["Win"] - 1)
    addr = ((b[:, None] * s["Hin"] + hi) * s["Win"] + wi) * ldx + c[None, :]
    return np.where(valid | clamp, addr, 0), valid


def _transform(s, p, dtype):
    """Coefficients of the input BatchNorm in float64 from the fp32 statistics, and per channel what fp32 arithmetic can move
    relu(x * sc + sh) by, as (a, b) with |delta| <= a |x sc| + b:
      mean = sum / count (3u), var = msq - mean^2 (u var + (6 mean^2 + 3 msq) u), sc = gamma * rsqrt(var + eps): relative
      rs = rv / 2 + 4u, sh = beta - mean sc: u |sh| + |mean sc| (rs + 3u), the fma and relu: u (|x sc| + |sh|)."""
    C = s["Cin"]
    cnt = float(s["B"] * s["Hin"] * s["Win"])
    mean, msq = p["in_stats"][:C] / cnt, p["in_stats"][C:] / cnt
    var = np.maximum(msq - mean * mean, 0.0)
    sc = p["in_gamma"] / np.sqrt(var + EPS)
    sh = p["in_beta"] - mean * sc
    rv = U + (6 * mean * mean + 3 * msq) * U / (var + EPS)
    rs = rv / 2 + 4 * U
    return sc, sh, rs + U, 2 * U * np.abs(sh) + np.abs(mean * sc) * (rs + 3 * U)


FAULTS = ("drop_last_chunk", "pad_neighbour", "xf_pad_relu_shift", "last_row_dup", "drop_tail_channels", "bias_per_slice",
          "stats_after_relu", "stats_after_rounding", "ldx_as_cin", "korder_misread", "replica0_only")


def fault_applies(fault, s, dtype):
    g = geometry(s)
    return {"drop_last_chunk": True,
            "pad_neighbour": s["pad"] > 0,
            "xf_pad_relu_shift": s["xf"] and s["pad"] > 0,
            "last_row_dup": g["M"] >= 2,
            "drop_tail_channels": s["N"] % 8 != 0,
            "bias_per_slice": s["split_k"] > 1 and s["bias"],
            "stats_after_relu": s["stats"] and s["relu"],
            # rounding errors are zero-mean: over many rows they hide inside a worst-case bound, which grows like M (M + K)
            "stats_after_rounding": s["stats"] and out_dtype(s, dtype) == "bfloat16" and g["M"] <= 64 and not s["affine"],
            "ldx_as_cin": s["ldx_pad"] > 0,
            "korder_misread": s["k_order"] == 1 and s["Cin"] > 8 * EPC[dtype],      # one chunk: the two orders are the same
            "replica0_only": s["stats"] and s["srep"] > 1}[fault]


def oracle(name, dtype, member=0, fault=None, rows=None, cols=None):
    """float64 result of the case: dict(y [M][N], bound [M][N], stats / stats_bound [R][2N] or None).  `fault` seeds one of
    FAULTS; rows / cols restrict the product to index subsets (the replica of the large cases)."""
    s, g, p = CASES[name], geometry(CASES[name]), inputs(name, dtype, member)
    M, N, K = g["M"], g["N"], g["K"]
    odt = out_dtype(s, dtype)
    c = C_BOUND[dtype]
    addr, valid = _gather_index(s, g, ldx=s["Cin"] if fault == "ldx_as_cin" else None, clamp=fault == "pad_neighbour")
    xg = np.where(valid | (fault == "pad_neighbour"), p["x"][addr], 0.0)
    extra_a = None
    if s["xf"]:
        sc, sh, ea, eb = _transform(s, p, dtype)
        ch = np.arange(K) % s["Cin"]
        pre = xg * sc[ch] + sh[ch]
        a = np.maximum(pre, 0.0)
        extra_a = ea[ch] * np.abs(xg * sc[ch]) + eb[ch] + (UB * a if dtype == "bfloat16" else 0.0)
        pad_val = np.maximum(sh[ch], 0.0)[None, :] if fault == "xf_pad_relu_shift" else 0.0
        xg, extra_a = np.where(valid | (fault == "pad_neighbour"), a, pad_val), np.where(valid, extra_a, 0.0)
    wl = p["w"][:, :K] if fault == "korder_misread" else p["wl"]
    if fault == "drop_last_chunk":
        xg = xg.copy(); xg[:, K - EPC[dtype]:] = 0.0
    if fault == "last_row_dup":
        xg = xg.copy(); xg[M - 1] = xg[M - 2]
    ri = np.arange(M) if rows is None else np.asarray(rows)
    ci = np.arange(N) if cols is None else np.asarray(cols)
    xg, wl = xg[ri], wl[ci]
    sel = lambda a: None if a is None else a[ci]
    bias, scale, shift = sel(p["bias"]), sel(p["scale"]), sel(p["shift"])
    acc = torch.from_numpy(xg) @ torch.from_numpy(wl).t()
    A = torch.from_numpy(np.abs(xg)) @ torch.from_numpy(np.abs(wl)).t()
    acc, A = acc.numpy(), A.numpy()
    E = (torch.from_numpy(extra_a[ri]) @ torch.from_numpy(np.abs(wl)).t()).numpy() if extra_a is not None else 0.0
    nb = (max(s["split_k"], 1) if fault == "bias_per_slice" else 1)
    v = acc + (nb * bias if bias is not None else 0.0)
    Tv = A + (np.abs(bias) if bias is not None else 0.0)
    T = Tv.copy()
    y = v.copy()
    if scale is not None:
        y, T, E = y * scale + shift, T * np.abs(scale) + np.abs(shift), E * np.abs(scale)
    y0 = p["y0"][p["lead"]:].reshape(M + 1, g["ldy"])[:M, :N][np.ix_(ri, ci)]
    if p["residual"] is not None:
        r = p["residual"][:, :N][np.ix_(ri, ci)]
        y, T = y + r, T + np.abs(r)
    if s["relu"]:
        y = np.maximum(y, 0.0)
    if s["accumulate"]:
        y, T = y + y0, T + np.abs(y0)
    bound = c * (K + 8) * U * T + E
    if odt == "bfloat16":
        bound = bound * (1 + UB) + UB * np.abs(y)
    if fault == "drop_tail_channels":
        keep = ci < N - N % 8
        y = np.where(keep[None, :], y, y0)
    out = dict(y=y, bound=bound, stats=None, stats_bound=None)
    if s["stats"] and rows is None and cols is None:
        sv = np.maximum(v, 0.0) if fault == "stats_after_relu" else _round(v, "bfloat16") if fault == "stats_after_rounding" else v
        R = max(s["srep"], 1)
        BM = route(s, dtype)[1]
        rep = np.zeros(M, dtype=np.int64) if fault == "replica0_only" else (np.arange(M) // BM) % R
        st, sb = p["stats0"].copy(), np.zeros((R, 2 * N))
        for r_ in range(R):
            mk = rep == r_
            st[r_, :N] += sv[mk].sum(0); st[r_, N:] += (sv[mk] ** 2).sum(0)
            # the M rows of a replica meet its old contents: M + 1 terms, still below M + 8
            sb[r_, :N] = c * ((K + 8) + (M + 8)) * U * (Tv[mk].sum(0) + np.abs(p["stats0"][r_, :N]))
            sb[r_, N:] = c * (2 * (K + 8) + 1 + (M + 8)) * U * ((Tv[mk] ** 2).sum(0) + np.abs(p["stats0"][r_, N:]))
        if fault == "replica0_only":      # the bound belongs to the true distribution over replicas
            true = oracle(name, dtype, member)
            sb = true["stats_bound"]
        out["stats"], out["stats_bound"] = st, sb
    return out


def ratios(got_y, got_stats, ref):
    """Largest |got - ref| / bound per compared quantity; anything not finite, or an error with a zero bound, counts as inf."""
    def worst(got, want, bound):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound)
        r = np.where(np.isfinite(r), r, np.inf)
        return float(r.max()) if r.size else 0.0
    out = {"y": worst(got_y, ref["y"], ref["bound"])}
    if ref["stats"] is not None:
        N = ref["stats"].shape[1] // 2
        out["sum"] = worst(got_stats[:, :N], ref["stats"][:, :N], ref["stats_bound"][:, :N])
        out["sumsq"] = worst(got_stats[:, N:], ref["stats"][:, N:], ref["stats_bound"][:, N:])
    return out


def split_y(s, dtype, ybuf, lead):
    """A flat y buffer -> (result [M][N], canary part as one vector: the lead, the pad columns, the guard row)."""
    g = geometry(s)
    M, N, ldy = g["M"], g["N"], g["ldy"]
    ybuf = np.asarray(ybuf)
    body = ybuf[lead:].reshape(M + 1, ldy)
    return body[:M, :N], np.concatenate([ybuf[:lead], body[:M, N:].reshape(-1), body[M]])


# ---- float32 / bf16 replica of the oracle: the arithmetic the bounds are derived for ---------------------------------------

def replica(name, dtype, rows=None, cols=None):
    """The case in the kernel's precisions on the CPU: a k-ordered fp32 fma chain over the (exact) products, fp32 epilogue in the
    header's order, statistics summed in fp32 row by row, the input transform in fp32 with the operand rounded to the storage
    type, the output rounded to its type.  Returns (y, stats)."""
    s, g, p = CASES[name], geometry(CASES[name]), inputs(name, dtype)
    M, N, K = g["M"], g["N"], g["K"]
    f = np.float32
    addr, valid = _gather_index(s, g)
    xg = np.where(valid, p["x"][addr], 0.0)
    if s["xf"]:
        C = s["Cin"]
        inv = f(1.0) / f(s["B"] * s["Hin"] * s["Win"])
        mean = p["in_stats"][:C].astype(f) * inv
        var = np.maximum(p["in_stats"][C:].astype(f) * inv - mean * mean, f(0))
        sc = p["in_gamma"].astype(f) / np.sqrt(var + f(EPS))
        sh = p["in_beta"].astype(f) - mean * sc
        ch = np.arange(K) % C
        a = np.maximum(xg.astype(f) * sc[ch] + sh[ch], f(0))
        xg = np.where(valid, _round(a.astype(np.float64), dtype), 0.0)
    ri = np.arange(M) if rows is None else np.asarray(rows)
    ci = np.arange(N) if cols is None else np.asarray(cols)
    xg, wl = xg[ri], p["wl"][ci]
    acc = np.zeros((len(ri), len(ci)), dtype=f)
    for k in range(K):
        acc = (acc.astype(np.float64) + xg[:, k, None] * wl[None, :, k]).astype(f)
    sel = lambda a: None if a is None else a[ci].astype(f)
    bias, scale, shift = sel(p["bias"]), sel(p["scale"]), sel(p["shift"])
    v = acc + bias if bias is not None else acc
    stats = None
    if s["stats"] and rows is None and cols is None:
        R, BM = max(s["srep"], 1), route(s, dtype)[1]
        stats = p["stats0"].astype(f)
        for m in range(M):
            r_ = (m // BM) % R
            stats[r_, :N] += v[m]; stats[r_, N:] += v[m] * v[m]
    y = v
    if scale is not None:
        y = y * scale + shift
    y0 = p["y0"][p["lead"]:].reshape(M + 1, g["ldy"])[:M, :N][np.ix_(ri, ci)].astype(f)
    if p["residual"] is not None:
        y = y + p["residual"][:, :N][np.ix_(ri, ci)].astype(f)
    if s["relu"]:
        y = np.maximum(y, f(0))
    if s["accumulate"]:
        y = y + y0
    return _round(y.astype(np.float64), out_dtype(s, dtype)), stats


# ---- refusals: (label, changes to the descriptor of REFUSAL_BASE, part of the message) ------------------------------------------
CASES["refusal_base"] = gemm(16, 16, 64, R_128x64 + (1,), "the accepted call every refusal is one change away from")
CASES["refusal_k72"] = gemm(16, 16, 72, R_128x64 + (0,), "the same with Cin = 72: no multiple of 128 bytes of channels")
RUNS += [(n, dt) for n in ("refusal_base", "refusal_k72") for dt in DTYPES]
REFUSALS = [
    ("null x", "base", dict(x=False), "null pointer"),
    ("null y", "base", dict(y=False), "null pointer"),
    ("bad dtype", "base", dict(dtype=7), "bad dtype"),
    ("Cin no multiple of a chunk", "base", dict(Cin=62), "Cin=62 must be a multiple"),
    ("ldx no multiple of a chunk", "base", dict(ldx=66), "ldx=66"),
    ("ldw no multiple of a chunk", "base", dict(ldw=66), "ldw=66"),
    ("sliding window past the row", "base", dict(ldx=32), "sliding-window input needs"),
    ("ldw below K", "base", dict(ldw=32), "leading dimensions too small"),
    ("negative stats_replicas", "base", dict(stats_replicas=-1), "bad stats_replicas"),
    ("ldy % 4", "base", dict(ldy=18), "ldy=18 must be a multiple of 4"),
    ("ldy < N", "base", dict(ldy=12), "ldy=12 must be a multiple of 4 and >= N=16"),
    ("B = 0", "base", dict(B=0), "bad geometry"),
    ("stride = 0", "base", dict(stride=0), "bad geometry"),
    ("Hin too large", "base", dict(Hin=32768), "spatial size too large"),
    ("input too large", "base", dict(B=1 << 20, Hin=16384), "input too large"),
    ("scale without shift", "base", dict(scale=True), "scale and shift must be given together"),
    ("k_order on Cin % 64", "k72", dict(k_order=1), "k_order=1 needs"),
    ("input transform without gamma", "base", dict(in_stats=True, in_beta=True, in_count=16.0), "input transform needs gamma, beta, count"),
    ("input transform without a count", "base", dict(in_stats=True, in_gamma=True, in_beta=True), "input transform needs gamma, beta, count"),
    ("input transform on a ragged K tile", "k72", dict(in_stats=True, in_gamma=True, in_beta=True, in_count=16.0),
     "the input transform needs Cin to be a multiple"),
    ("split-K with relu", "base", dict(split_k=2, Cin=128, ldx=128, ldw=128, out_dtype=0, relu=1), "split_k=2 needs"),
    ("split-K with K not divisible", "base", dict(split_k=2, Cin=96, ldx=96, ldw=96, out_dtype=0), "split_k=2 needs"),
    ("split-K into bf16", "base", dict(split_k=2, Cin=128, ldx=128, ldw=128, out_dtype=1), "split_k=2 needs"),
    ("split-K 13", "base", dict(split_k=13, Cin=64 * 13, ldx=64 * 13, ldw=64 * 13, out_dtype=0), "split_k=13 needs"),
]
# st_conv_batch: (label, n, member 1's changes, message)
BATCH_REFUSALS = [("n = 0", 0, {}, "1..12 problems per launch"), ("n = 13", 13, {}, "1..12 problems per launch"),
                  ("members of different shape", 2, dict(N=12), "problem 1 differs in shape or options from problem 0"),
                  ("a member that is refused itself", 2, dict(ldy=18), "ldy=18")]


def refusal_descriptor(base, changes, dtype):
    return dict(descriptor(CASES["refusal_" + base], dtype), **changes)
