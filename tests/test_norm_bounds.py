"""RMSNorm / LayerNorm (csrc/rmsnorm.hip) against an fp64 reference with an a-priori, per-element bound.

The assert_close tolerances of tests/test_gpu_models.py accept a LayerNorm dx without its mean(g) term, and at (3, 8192)
a dx with no reduction at all (test_old_tolerance_misses_a_dropped_mean keeps the figures on record).  Here y, the saved
mean / rstd, dx, dw and db are each held to a bound derived from the kernels' dataflow: one U = 2^-8 term at each
bf16 store (y, dx; the fused ADD backward rounds dx + dres once), and fp32 terms written as sums of absolute values:
the row sum behind mean / rstd, that error carried into xhat, the reductions mean(gw) and mean(gw * xhat), the
fmaf(xhat, w, bias) cancellation, the accumulation over rows of dw / db (rows of a workgroup, the wave combine, the two
levels of partial_colsum) and 2 ulp for rsqrtf.  No bf16 term on dw, db, mean, rstd.  An fp32 sum is charged
gamma(k) = k 2^-24 / (1 - k 2^-24) times the sum of absolute values, k the longest chain of additions a term passes
through.  The statistic is max |got - ref| / bound and the assertion is <= 1.0.  A path that rounds to bf16 twice (the
unfused add + norm: bf16 dx of the norm, then autograd's bf16 add of the residual gradient) is charged both roundings.

Layout: the oracle, an fp32 emulation of the kernels in their lane layout (CPU tests: the emulation is inside the
bound, injected defects are outside), the GPU cases through rms_norm / layer_norm / add_rms_norm / add_layer_norm, and
direct ctypes calls (guard patterns, plx_partial_colsum, argument validation).

Largest measured ratio per kernel family on an MI355X (NORM_RATIO lines of the GPU cases; the fp32 emulation's over the
CPU-sized cases in brackets):

    family         y              mean           rstd           dx             dw             db
    rms            0.996 (0.996)  -              0.230 (0.261)  0.996 (0.996)  0.166 (0.165)  -
    add_rms        0.996 (0.996)  -              0.230 (0.261)  0.996 (0.996)  0.147 (0.187)  -
    ln_wave        0.996 (0.996)  0.099 (0.099)  0.230 (0.261)  0.995 (0.995)  0.082 (0.082)  0.053 (0.079)
    add_ln_wave    0.996 (0.996)  0.087 (0.087)  0.230 (0.261)  0.996 (0.996)  0.082 (0.087)  0.050 (0.072)
    ln_wg          0.996 (0.996)  0.158 (0.158)  0.230 (0.261)  0.995 (0.995)  0.086 (0.086)  0.092 (0.092)
    partial_colsum 0.200 (direct calls, against gamma(chain) * sum |p|)

rms / add_rms: rms_fwd_kernel, rms_bwd_kernel; ln_wave / add_ln_wave: ln_fwd_wave_kernel, ln_bwd_wave_kernel
(d <= 1024); ln_wg: ln_fwd_kernel, ln_bwd_kernel (the unfused add_layer_norm above d = 1024 included); every family with
partial_colsum behind dw / db.  y and dx sit at the bf16 rounding itself.  The fp32 quantities use a tenth to a quarter
of bounds that are worst case in every sign; db reaches 0.05 only with a gradient of one sign (kind 'posg': with random
signs the partial sums are ~ sqrt(rows), the bound ~ rows, measured 0.004), and is required to be exact wherever fp32
holds every partial sum exactly (most cases of a few rows).
"""
import functools
import math
import zlib
from collections import namedtuple

import pytest
import torch

U = 2.0 ** -8            # bf16 round-to-nearest unit roundoff
E = 2.0 ** -24           # fp32 unit roundoff
RSQ = 4 * E              # rsqrtf: 2 ulp
GUARD16, GUARD32 = 0x7B7B, 0x7B7B7B7B
QUANT = ("y", "mean", "rstd", "dx", "dw", "db")

Case = namedtuple("Case", "op rows d kind eps")
OPS = ("rms", "ln", "add_rms", "add_ln")


def _mk(op, rows, d, kind="gauss", eps=1e-5) -> Case:
    return Case(op, rows, d, kind, eps)


def _id(c: Case) -> str:
    return f"{c.op}-{c.rows}x{c.d}-{c.kind}" + ("" if c.eps == 1e-5 else f"-eps{c.eps:g}")


def _is_ln(op) -> bool:
    return op.endswith("ln")


def _is_add(op) -> bool:
    return op.startswith("add")


# ------------------------------------------------------------------------------- the launch geometry of rmsnorm.hip
def _path(op, d) -> str:
    """'wave1' / 'wave2' (ln_vpl, rmsnorm.hip:508: one wave per row, 1 or 2 vectors per lane) or 'wg' (a 256-thread
    workgroup per row: every RMSNorm kernel, LayerNorm above d = 1024)."""
    if _is_ln(op) and d <= 1024 and d % 8 == 0:
        return "wave1" if d <= 512 else "wave2"
    return "wg"


def _fused(op, d) -> bool:
    """add_layer_norm is one kernel on the wave path only (ops/rmsnorm.py add_layer_norm); add_rms_norm always."""
    return op == "add_rms" or (op == "add_ln" and d <= 1024)


def _family(op, d) -> str:
    if not _is_ln(op):
        return op
    if _path(op, d) == "wg":
        return "ln_wg"
    return "add_ln_wave" if op == "add_ln" else "ln_wave"


def _bwd_blocks(path, rows) -> int:
    """plx_rms_bwd_blocks / plx_ln_bwd_blocks (:495, :529)."""
    return min(rows, 1024) if path == "wg" else min((rows + 3) // 4, 1024)


def _row_depth(path, d) -> int:
    """Longest chain of fp32 additions in a row reduction: 8 elements of each of the lane's vectors in sequence, the
    6-step shuffle tree, and in block_sum (:35) the 4 per-wave values in sequence; never more than d terms."""
    lanes = 256 if path == "wg" else 64
    nv = -(-(d // 8) // lanes)
    return min(d, 8 * nv + 6 + (4 if path == "wg" else 0))


def _colsum_depth(nb) -> int:
    """partial_colsum_kernel (:419): a thread adds up to 16 of a split's 64 rows, 4 row groups are added in sequence;
    the last arriver adds ceil(R / 4) split sums per thread and again the 4 groups."""
    n1 = min(nb, 64)
    R = -(-nb // 64)
    return -(-n1 // 4) + min(4, n1) + -(-R // 4) + min(4, R)


def _param_depth(path, rows) -> int:
    """Chain of a dw / db column: the rows one workgroup (:111, :227) or one wave (:366) accumulates in registers, the
    4 waves of a wave-path workgroup added in order (:404), then partial_colsum."""
    nb = _bwd_blocks(path, rows)
    per = -(-rows // nb) if path == "wg" else -(-rows // (4 * nb)) + 3
    return per + _colsum_depth(nb)


def _gamma(k):
    return k * E / (1 - k * E)


def _eps32(eps) -> float:
    """The kernels take eps as a float argument."""
    return float(torch.tensor(eps, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------------ the cases
_D_EDGES = [8, 504, 512, 520, 1016, 1024, 1032, 2048, 2056, 4096, 8192]
_FEW_ROWS = [1, 2, 3, 5]
EDGE = [_mk(op, _FEW_ROWS[(i + j) % 4], d) for j, op in enumerate(OPS) for i, d in enumerate(_D_EDGES)]
# rows on both sides of each grid cap: 1024 workgroups (rms_bwd, ln_bwd), 4096 (rms_fwd, ln_fwd), 1024 x 4 waves
# (ln_bwd_wave), 8192 x 4 waves (ln_fwd_wave); d = 64 / 520 are wave-path LayerNorm shapes, 1032 the workgroup kernels
STRIDE = ([_mk(op, r, d) for op in OPS for d in (64, 1032) for r in (1024, 1025, 2049 + 7, 4096, 4097)]
          + [_mk(op, r, d) for op in ("ln", "add_ln") for d in (64, 520) for r in (4096, 4097, 4099)]
          + [_mk(op, r, d) for op in ("ln", "add_ln") for d in (8, 520) for r in (32768, 32771)])
_KIND_SHAPES = [(5, 520), (7, 1032), (3, 2056), (1025, 64)]
KINDS = [_mk(op, r, d, k) for op in OPS for k in ("off20", "off300", "degen", "spike", "mixedw")
         for r, d in _KIND_SHAPES]
# a gradient of one sign: the partial sums of db (and of dw's |g| weights) grow like the sums of absolute values the
# bounds are written in, where a gradient of random signs uses a few percent of them
KINDS += [_mk(op, r, d, "posg") for op in OPS for r, d in [(1025, 64), (2049 + 7, 1032)]]
EPS = [_mk(op, r, d, "degen", e) for op in OPS for e in (1e-6, 1e-2) for r, d in _KIND_SHAPES[:2]]
CASES = list(dict.fromkeys(EDGE + STRIDE + KINDS + EPS))


def _cpu_sized(c: Case) -> Case:
    """The case the CPU tests run: the large-row cases cut to rows that still give a workgroup several rows."""
    cap = 4100 if c.d <= 64 else 1100
    return c if c.rows <= cap else c._replace(rows=cap + c.rows % 4)


CPU_CASES = list(dict.fromkeys(_cpu_sized(c) for c in CASES))

Inputs = namedtuple("Inputs", "x res w b gy gs")


def _inputs(c: Case) -> Inputs:
    """bf16 x, res, gy, gs [rows, d] and fp32 w, b [d] of a case (CPU tensors).  The norm's input is x for the plain
    ops and s = bf16(x + res) for the add ops."""
    gen = torch.Generator().manual_seed(zlib.crc32(_id(c).encode()))
    rnd = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    rows, d, ln = c.rows, c.d, _is_ln(c.op)
    x, res = 3.0 * rnd(rows, d), 0.5 * rnd(rows, d)
    w, b = torch.rand(d, generator=gen) + 0.5, rnd(d)
    gy, gs = rnd(rows, d), rnd(rows, d)
    if c.kind == "off20":
        x += 20.0
    elif c.kind == "off300":          # bf16 spacing 2 at 300: coarser than the spread
        x = x / 3.0 + 300.0
    elif c.kind == "degen":           # rstd = 1 / sqrt(eps): an all-zero row, and for LayerNorm a constant row
        x[0], res[0] = 0.0, 0.0
        if ln and rows > 1:
            x[rows - 1], res[rows - 1] = 2.5, 0.0
    elif c.kind == "spike":           # one 1e4 in an otherwise unit row
        x = x / 3.0
        for r in range(0, rows, max(1, rows // 3)):
            x[r, (7 * r + 3) % d] = 1e4
    elif c.kind == "mixedw":          # weights of both signs; bias = -w * xhat of row 0 on every other column
        w = rnd(d)
        src = (x[0].bfloat16() + res[0].bfloat16()).double() if _is_add(c.op) else x[0].bfloat16().double()
        cen = src - src.mean() if ln else src
        xh = cen * ((cen * cen).mean() + c.eps).rsqrt()
        b[::2] = (-w.double() * xh).float()[::2]
    elif c.kind == "posg":
        gy = gy.abs()
    bf = lambda t: t.to(torch.bfloat16)  # noqa: E731
    return Inputs(bf(x), bf(res) if _is_add(c.op) else None, w, b if ln else None, bf(gy),
                  bf(gs) if _is_add(c.op) else None)


# ------------------------------------------------------------------------------------------------------ the oracle
def _oracle(op, x, res, w, b, gy, gs, eps, fused=None):
    """fp64 reference and per-element bounds of y, mean, rstd, dx (the gradient of x and of res: the norm's dx plus gs
    when given), dw, db, and the bf16 sum s.  Runs on the device of its inputs.  ``fused`` False: dx is rounded to
    bf16 by the norm and once more by autograd's add of gs."""
    ln, add = _is_ln(op), _is_add(op)
    rows, d = x.shape
    fused = _fused(op, d) if fused is None else fused
    path = _path(op, d)
    K, Kp = _row_depth(path, d), _param_depth(path, rows)
    eps = _eps32(eps)
    s = x + res if add else None                       # torch's bf16 add: the fp32 sum rounded once, as :64 / :291
    X = (s if add else x).double()
    W, G = w.double(), gy.double()
    ksum = lambda t: t.sum(-1, keepdim=True)  # noqa: E731
    if ln:
        # s1 += xs (:164, :297) then mean = sum * inv_d (:168, :300): the sum, inv_d = fl(1 / d) and the product
        mean = ksum(X) / d
        b_mean = _gamma(K + 2) * ksum(X.abs()) / d
        C = X - mean
        b_c = b_mean + E * (C.abs() + b_mean)          # c = fl(xs - mean) (:176, :307)
    else:
        mean, b_mean = None, None
        C = X
        b_c = torch.zeros_like(X)
    # s2 = sum fmaf(c, c, s2) (:70, :177, :308): the error of c carried into the squares, the sum, then / d (or
    # * inv_d) and + eps; relative to var + eps, through rsqrtf (:74, :181, :312) at half weight
    ss = ksum(C * C)
    v = ss / d + eps
    e_v = (ksum(b_c * (2 * C.abs() + b_c)) * (1 + _gamma(K + 3)) + _gamma(K + 3) * ss) / d / v
    e_rstd = 0.5 * e_v / (1 - e_v.clamp(max=0.5)) + RSQ
    rstd = v.rsqrt()
    b_rstd = rstd * e_rstd
    # xhat = fl(c * rstd) (:80, :192, :223, :323, :362), forward and backward alike
    XH = C * rstd
    b_xh = (rstd * b_c + XH.abs() * (e_rstd + E)) * (1 + e_rstd) * (1 + E)
    # y = bf16(fmaf(xhat, w, bias)) (:192, :323) / bf16(fl(xhat * w)) (:80): the error of xhat is absolute, so a
    # bias that cancels w * xhat does not shrink it
    Y = XH * W + (b.double() if ln else 0.0)
    b_y = U * Y.abs() + (1 + U) * (W.abs() * b_xh + E * (Y.abs() + W.abs() * b_xh))
    # backward: gw = fl(g * w); sg += gw, sgx = fmaf(gw, xhat, sgx) (:225-226, :364-365; :110 for RMSNorm)
    GW = G * W
    if ln:
        mg = ksum(GW) / d
        b_mg = _gamma(K + 3) * ksum(GW.abs()) / d
    else:
        mg, b_mg = torch.zeros_like(rstd), torch.zeros_like(rstd)
    mgx = ksum(GW * XH) / d
    b_mgx = (ksum(GW.abs() * b_xh) + _gamma(K + 3) * ksum(GW.abs() * (XH.abs() + b_xh))) / d
    # inner = gw - mg - xhat * mgx (:127, :240, :381, :384): gw, both means, the product and two subtractions
    inner = GW - mg - XH * mgx
    b_in = (3 * E * GW.abs() + 2 * E * mg.abs() + b_mg + XH.abs() * b_mgx + (mgx.abs() + b_mgx) * b_xh
            + 2 * E * (XH * mgx).abs())
    DX = rstd * inner
    b_dx32 = rstd * b_in * (1 + e_rstd + E) + (e_rstd + E) * DX.abs()
    if gs is None:
        OUT = DX
        b_dx = U * OUT.abs() + (1 + U) * (b_dx32 + E * OUT.abs())
    elif fused:
        # fl(fl(rstd * inner) + dres) (:128) or one fmaf (:381), then one bf16 rounding
        OUT = DX + gs.double()
        b_dx = U * OUT.abs() + (1 + U) * (b_dx32 + E * (DX.abs() + OUT.abs()))
    else:
        OUT = DX + gs.double()
        b_n = U * DX.abs() + (1 + U) * (b_dx32 + E * DX.abs())
        b_dx = U * OUT.abs() + (1 + U) * b_n
    # dw = sum_r fmaf(g, xhat, dw) (:111, :227, :366), db = sum_r g (:228, :367): no bf16 anywhere
    dw = (G * XH).sum(0)
    b_dw = (G.abs() * b_xh).sum(0) + _gamma(Kp) * (G.abs() * (XH.abs() + b_xh)).sum(0)
    ref = dict(y=Y, rstd=rstd[:, 0], dx=OUT, dw=dw)
    bound = dict(y=b_y, rstd=b_rstd[:, 0], dx=b_dx, dw=b_dw)
    if ln:
        # every g of a column is a multiple of q, the bf16 ulp of its smallest non-zero |g|, and so is every partial
        # sum; while sum |g| < 2^24 q they all fit an fp32 significand and no addition rounds: db must be exact
        A = G.abs()
        q = torch.where(A > 0, torch.exp2(torch.floor(torch.log2(A)) - 7), math.inf).amin(0)
        b_db = torch.where(A.sum(0) < 2.0 ** 24 * q, torch.zeros_like(q), _gamma(Kp) * A.sum(0))
        ref.update(mean=mean[:, 0], db=G.sum(0))
        bound.update(mean=b_mean[:, 0], db=b_db)
    return ref, bound, s


def _ratio(got, ref, bound) -> float:
    """max |got - ref| / bound.  A bound of exactly 0 means the element must be exact; NaN must sit exactly where
    the reference has it."""
    got = got.double().reshape(ref.shape)
    nan = ref.isnan()
    if not torch.equal(got.isnan(), nan):
        return math.inf
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    r = torch.where(nan, torch.zeros_like(r), r).nan_to_num(nan=math.inf)
    return float(r.max()) if r.numel() else 0.0


def _ratios(got: dict, ref: dict, bound: dict, names=None) -> dict:
    names = [n for n in QUANT if n in ref] if names is None else names
    return {n: _ratio(got[n].to(ref[n].device), ref[n], bound[n]) for n in names}


def _fmt(r: dict) -> str:
    return " ".join(f"{n}={x:.3f}" for n, x in r.items())


def _same_bits(a, b) -> bool:
    """bf16 tensors equal element for element, a NaN matching any NaN."""
    return bool(torch.equal(a.isnan(), b.isnan())) and bool(torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0)))


Data = namedtuple("Data", "inp ref bound s")


def _on(inp: Inputs, dev) -> Inputs:
    return Inputs(*(None if t is None else t.to(dev) for t in inp))


@functools.lru_cache(maxsize=2)
def _data(c: Case, dev="cpu") -> Data:
    """Inputs (on ``dev``), fp64 reference and bounds of a case, shared read-only by the tests of the case."""
    inp = _on(_inputs(c), dev)
    ref, bound, s = _oracle(c.op, *inp, c.eps)
    return Data(inp, ref, bound, s)


# ----------------------------------------------------------------------------- fp32 emulation of the kernels (CPU)
_F32 = torch.float32


def _bf(t):
    return t.to(torch.bfloat16).to(_F32)


def _lane_sum(a, b, path):
    """sum_k fmaf(a_k, b_k, acc) (b None: acc += a_k) over a row in the kernels' order: lane l owns vectors l,
    l + lanes, ..., 8 elements each in sequence, then the xor-shuffle tree and block_sum's 4 waves in order."""
    rows, d = a.shape
    lanes = 256 if path == "wg" else 64
    nv = -(-(d // 8) // lanes)
    p = a.double() * b.double() if b is not None else a.double()
    p = torch.nn.functional.pad(p, (0, nv * lanes * 8 - d)).view(rows, nv, lanes, 8)
    acc = torch.zeros(rows, lanes, dtype=_F32)
    for j in range(nv):
        for k in range(8):
            acc = (acc.double() + p[:, j, :, k]).to(_F32)
    acc = acc.view(rows, lanes // 64, 64)
    idx = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., idx ^ off]
    acc = acc[..., 0]
    tot = torch.zeros(rows, dtype=_F32)
    for i in range(acc.shape[1]):
        tot = tot + acc[:, i]
    return tot[:, None]


def _emulate(op, x, res, w, b, gy, gs, eps, defect=None):
    """The kernels' dataflow in fp32 torch with bf16 roundings at the y and dx stores.  ``defect`` injects one of:
    'nomg' (dx without mean(g)), 'nomgx' (dx without xhat * mean(g * xhat), for RMSNorm its only mean term), 'nomeans'
    (both), 'row' (dw / db without row rows // 2), 'part' (dw without one workgroup's partial row), 'tail' (the last
    vector of each row left out of the variance), 'onepass' (variance as E[x^2] - E[x]^2), 'normx' (an add op
    normalising x instead of s)."""
    ln, add = _is_ln(op), _is_add(op)
    rows, d = x.shape
    path = _path(op, d)
    eps = torch.tensor(eps, dtype=_F32)
    s = x + res if add else None
    X = (x if (not add or defect == "normx") else s).to(_F32)
    inv_d = torch.tensor(1.0, dtype=_F32) / torch.tensor(float(d), dtype=_F32)
    mean = _lane_sum(X, None, path) * inv_d if ln else None
    C = X - mean if ln else X
    Cv = C.clone()
    if defect == "tail":
        Cv[:, d - 8:] = 0.0
    if defect == "onepass":
        var = _lane_sum(X, X, path) * inv_d - mean * mean
    elif ln:
        var = _lane_sum(Cv, Cv, path) * inv_d
    else:
        var = _lane_sum(Cv, Cv, path) / torch.tensor(float(d), dtype=_F32)
    rstd = (var + eps).rsqrt()
    XH = C * rstd
    y = _bf((XH.double() * w.double() + b.double()).to(_F32)) if ln else _bf(XH * w)
    G = gy.to(_F32)
    GW = G * w
    zero = torch.zeros(rows, 1, dtype=_F32)
    if ln:
        mg = zero if defect in ("nomg", "nomeans") else _lane_sum(GW, None, path) * inv_d
        mgx = zero if defect in ("nomgx", "nomeans") else _lane_sum(GW, XH, path) * inv_d
        dx32 = rstd * (GW - mg - XH * mgx)
    else:
        md = zero if defect in ("nomgx", "nomeans") else _lane_sum(GW, XH, path) / torch.tensor(float(d), dtype=_F32)
        dx32 = rstd * (GW - XH * md)
    dx = _bf(dx32 + gs.to(_F32)) if gs is not None else _bf(dx32)
    # parameter gradients: the partial row of the workgroup that owns each row, then the column sum
    nb = _bwd_blocks(path, rows)
    r = torch.arange(rows)
    blk = r % nb if path == "wg" else (r % (4 * nb)) // 4
    tw, tb = G * XH, G.clone()
    if defect == "row":
        tw[rows // 2], tb[rows // 2] = 0.0, 0.0
    pw = torch.zeros(nb, d, dtype=_F32).index_add_(0, blk, tw)
    pb = torch.zeros(nb, d, dtype=_F32).index_add_(0, blk, tb)
    if defect == "part":
        pw[nb // 2] = 0.0
    out = dict(y=y, rstd=rstd[:, 0], dx=dx, dw=pw.sum(0))
    if ln:
        out.update(mean=mean[:, 0], db=pb.sum(0))
    return out, s


def _emu(c: Case, defect=None):
    d = _data(c)
    return _emulate(c.op, *d.inp, c.eps, defect)[0]


@pytest.mark.parametrize("case", CPU_CASES, ids=_id)
def test_emulation_stays_inside_the_bound(case):
    """The bounds are satisfiable: a correct fp32 computation in the kernels' order, with their bf16 roundings, has
    ratio <= 1 for every quantity of every case (the large-row cases cut to CPU size)."""
    d = _data(case)
    r = _ratios(_emu(case), d.ref, d.bound)
    print(f"NORM_RATIO emu {_family(case.op, case.d)} {_id(case)}: {_fmt(r)}")
    assert all(x <= 1.0 for x in r.values()), r


_DEFECTS = {
    # defect: (quantities that must leave their bound, cases)
    "nomg": (("dx",), [_mk("ln", 37, 768, "off20"), _mk("ln", 3, 8192, "off20"), _mk("ln", 5, 1032),
                       _mk("add_ln", 5, 520), _mk("ln", 2, 8)]),
    "nomgx": (("dx",), [_mk("ln", 37, 768, "off20"), _mk("ln", 3, 8192, "off20"), _mk("add_ln", 5, 520),
                        _mk("rms", 37, 768), _mk("rms", 3, 8192), _mk("add_rms", 5, 520), _mk("rms", 2, 8)]),
    "row": (("dw", "db"), [_mk("ln", 5000, 768, "off20"), _mk("ln", 1025, 1032), _mk("add_ln", 4100, 64)]),
    "row_rms": (("dw",), [_mk("rms", 5000, 768), _mk("add_rms", 1025, 64)]),
    "part": (("dw",), [_mk("ln", 5000, 768, "off20"), _mk("ln", 2056, 1032), _mk("rms", 2056, 64),
                       _mk("add_rms", 1025, 1032)]),
    "tail": (("rstd",), [_mk("ln", 37, 768, "off20"), _mk("ln", 3, 2056), _mk("rms", 5, 520), _mk("add_rms", 3, 8192),
                         _mk("add_ln", 5, 1016)]),
    "onepass": (("rstd",), [_mk("ln", 37, 768, "off300"), _mk("ln", 7, 1032, "off300"),
                            _mk("add_ln", 5, 520, "off300")]),
    "normx": (("y", "rstd", "dx", "dw"), [_mk("add_rms", 5, 520), _mk("add_ln", 5, 520), _mk("add_rms", 7, 1032)]),
}


@pytest.mark.parametrize("defect,case", [(k, c) for k, (_, cs) in _DEFECTS.items() for c in cs],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_injected_defect_exceeds_the_bound(defect, case):
    d = _data(case)
    r = _ratios(_emu(case, defect.split("_")[0]), d.ref, d.bound)
    print(f"{defect} {_id(case)}: {_fmt(r)}")
    for name in _DEFECTS[defect][0]:
        assert r[name] > 1.0, (name, r)


def test_old_tolerance_misses_a_dropped_mean():
    """Why this file exists: with the inputs and the assert_close tolerances of test_layernorm_matches_fp32 (rtol 3e-2,
    atol 3e-2 * max |dx|), a LayerNorm dx without its mean(g) term passes at (37, 768), and at (3, 8192) a dx with no
    mean term at all passes; both are many times the per-element bound."""
    for rows, d, defect in ((37, 768, "nomg"), (3, 8192, "nomeans")):
        gen = torch.Generator().manual_seed(0)
        x = (torch.randn(rows, d, generator=gen) * 3 + 20).to(torch.bfloat16)
        w, b = torch.rand(d, generator=gen) + 0.5, torch.randn(d, generator=gen)
        g = torch.randn(rows, d, generator=gen).to(torch.bfloat16)
        xr = x.float().requires_grad_()
        torch.nn.functional.layer_norm(xr, (d,), w, b, 1e-5).backward(g.float())
        got = _emulate("ln", x, None, w, b, g, None, 1e-5, defect)[0]
        torch.testing.assert_close(got["dx"], xr.grad, rtol=3e-2, atol=3e-2 * float(xr.grad.abs().max()))
        ref, bound, _ = _oracle("ln", x, None, w, b, g, None, 1e-5)
        r = _ratio(got["dx"], ref["dx"], bound["dx"])
        ok = _ratio(_emulate("ln", x, None, w, b, g, None, 1e-5)[0]["dx"], ref["dx"], bound["dx"])
        print(f"({rows}, {d}) {defect}: passes assert_close, bound ratio {r:.1f} (without the defect {ok:.3f})")
        assert r > 1.0 and ok <= 1.0


# ------------------------------------------------------------------------------------- GPU: through the public ops
def _apply(op, x, res, w, b, eps):
    from polyaxon_amd.ops import rmsnorm as R

    if op == "rms":
        return None, R.rms_norm(x, w, eps)
    if op == "ln":
        return None, R.layer_norm(x, w, b, eps)
    if op == "add_rms":
        return R.add_rms_norm(x, res, w, eps)
    return R.add_layer_norm(x, res, w, b, eps)


def _run(op, inp: Inputs, eps, backprop="both"):
    """Forward and backward through the public op.  ``backprop``: 'both', 'y' or 's' (the add ops' branches)."""
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_()  # noqa: E731
    x, res, w, b = leaf(inp.x), leaf(inp.res), leaf(inp.w), leaf(inp.b)
    s, y = _apply(op, x, res, w, b, eps)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    got = dict(y=y.detach(), s=None if s is None else s.detach())
    saved = y.grad_fn.saved_tensors          # (x or s, w, [mean,] rstd) of the norm's autograd node
    got["rstd"] = saved[-1].clone()
    if _is_ln(op):
        got["mean"] = saved[-2].clone()
    if not _is_add(op):
        y.backward(inp.gy)
    elif backprop == "both":
        torch.autograd.backward([s, y], [inp.gs, inp.gy])
    elif backprop == "y":
        y.backward(inp.gy)
    else:
        s.backward(inp.gs)
    got.update(dx=x.grad, dres=None if res is None else res.grad, dw=w.grad, db=None if b is None else b.grad)
    return got


def _check(op, got, ref, bound, s, tag):
    r = _ratios(got, ref, bound)
    print(f"NORM_RATIO gpu {_family(op, got['y'].shape[-1])} {tag}: {_fmt(r)}")
    assert all(x <= 1.0 for x in r.values()), (tag, r)
    if _is_add(op):
        assert _same_bits(got["s"], s), tag
        rr = _ratio(got["dres"], ref["dx"], bound["dx"])
        assert rr <= 1.0, (tag, "dres", rr)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_norm_within_bound(cuda, case):
    """y, the saved mean / rstd, dx (for the add ops: s bitwise, and the gradient of both inputs with both output
    gradients flowing), dw and db of every case within their per-element bounds."""
    d = _data(case, cuda)
    got = _run(case.op, d.inp, case.eps)
    _check(case.op, got, d.ref, d.bound, d.s, _id(case))
    if case.kind == "degen":
        # an all-zero row: rstd = 1 / sqrt(eps) to the rsqrtf allowance
        want = 1.0 / math.sqrt(_eps32(case.eps))
        assert abs(float(got["rstd"][0]) - want) <= RSQ * want


_NAN_SHAPES = [(5, 520), (6, 1032), (1030, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["x", "gy"])
@pytest.mark.parametrize("case", [_mk(op, r, d) for op in OPS for r, d in _NAN_SHAPES], ids=_id)
def test_nan_stays_in_its_row(cuda, case, where):
    """One NaN in x makes exactly that row of y and dx (and that rstd / mean) NaN, every column of dw NaN and leaves db
    alone; one NaN in dy makes that row of dx and that column of dw and db NaN.  Everything else stays inside its
    bound (_ratio demands NaN exactly where the fp64 reference has it)."""
    inp = _inputs(case)
    r0, c0 = case.rows // 2, (3 * case.d) // 4 + 1
    getattr(inp, where)[r0, c0] = math.nan
    inp = _on(inp, cuda)
    ref, bound, s = _oracle(case.op, *inp, case.eps)
    rows = torch.arange(case.rows, device=cuda)
    assert bool(ref["dx"].isnan().all(1).eq(rows == r0).all()) and bool(ref["dx"].isnan().any(1).eq(rows == r0).all())
    assert bool(ref["y"].isnan().any(1).eq((rows == r0) & (where == "x")).all())
    assert int(ref["dw"].isnan().sum()) == (case.d if where == "x" else 1)
    if _is_ln(case.op):
        assert int(ref["db"].isnan().sum()) == (0 if where == "x" else 1)
    got = _run(case.op, inp, case.eps)
    _check(case.op, got, ref, bound, s, f"{_id(case)} nan-in-{where}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [_mk(op, r, d) for op in ("add_rms", "add_ln") for r, d in [(5, 520), (1030, 64)]],
                         ids=_id)
def test_add_backward_branches(cuda, case):
    """The three branches of _AddRMSNorm / _AddLayerNorm.backward: a gradient through y only (the plain backward
    kernel), through s only (dx is gs, the parameters get none), and through both (covered by every other case)."""
    d = _data(case, cuda)
    got = _run(case.op, d.inp, case.eps, "y")
    ref, bound, s = _oracle(case.op, *d.inp._replace(gs=None), case.eps)
    _check(case.op, got, ref, bound, s, f"{_id(case)} y-only")
    got = _run(case.op, d.inp, case.eps, "s")
    assert torch.equal(got["dx"], d.inp.gs) and torch.equal(got["dres"], d.inp.gs)
    assert got["dw"] is None and got["db"] is None
    got = _run(case.op, d.inp, case.eps, "both")
    _check(case.op, got, d.ref, d.bound, d.s, f"{_id(case)} both")


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("d", [100, 8200])
def test_unsupported_width_takes_the_reference_path(cuda, op, d):
    """d % 8 != 0 and d > 8192: the PyTorch composition, bit for bit, and no native autograd node."""
    from polyaxon_amd.ops import rmsnorm as R

    c = _mk(op, 3, d)
    inp = _on(_inputs(c), cuda)

    def direct():
        x, w = inp.x.clone().requires_grad_(), inp.w.clone().requires_grad_()
        b = None if inp.b is None else inp.b.clone().requires_grad_()
        res = None if inp.res is None else inp.res.clone().requires_grad_()
        s = x + res if res is not None else x
        y = R.layer_norm_reference(s, w, b, c.eps) if _is_ln(op) else R.rms_norm_reference(s, w, c.eps)
        if res is not None:
            torch.autograd.backward([s, y], [inp.gs, inp.gy])
        else:
            y.backward(inp.gy)
        return y.detach(), x.grad, w.grad, None if b is None else b.grad

    leaf = lambda t: None if t is None else t.clone().requires_grad_()  # noqa: E731
    x, res, w, b = leaf(inp.x), leaf(inp.res), leaf(inp.w), leaf(inp.b)
    s, y = _apply(op, x, res, w, b, c.eps)
    assert y.dtype == torch.bfloat16
    for t in (y,) if s is None else (s, y):
        assert not type(t.grad_fn).__name__.startswith("_"), type(t.grad_fn).__name__
    if s is None:
        y.backward(inp.gy)
    else:
        torch.autograd.backward([s, y], [inp.gs, inp.gy])
    yr, dxr, dwr, dbr = direct()
    assert torch.equal(y, yr) and torch.equal(x.grad, dxr) and torch.equal(w.grad, dwr)
    if b is not None:
        assert torch.equal(b.grad, dbr)
    if s is not None:
        assert torch.equal(s, inp.x + inp.res) and torch.equal(res.grad, dxr)
    # and it is a norm: y and dx inside the bounds of a path that rounds dx twice
    ref, bound, _ = _oracle(op, *inp, c.eps, fused=False)
    r = _ratios(dict(y=y, dx=x.grad), ref, bound, ("y", "dx"))
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.gpu
def test_add_layer_norm_above_the_wave_path_is_unfused(cuda):
    """add_layer_norm at d = 1032: a torch add and the workgroup-per-row LayerNorm, inside the bounds."""
    c = _mk("add_ln", 7, 1032)
    d = _data(c, cuda)
    x, res = d.inp.x.clone().requires_grad_(), d.inp.res.clone().requires_grad_()
    s, y = _apply(c.op, x, res, d.inp.w, d.inp.b, c.eps)
    assert type(s.grad_fn).__name__ == "AddBackward0" and type(y.grad_fn).__name__ == "_LayerNormBackward"
    c = _mk("add_ln", 7, 1024)
    s, y = _apply(c.op, *(t.clone().requires_grad_() for t in _on(_inputs(c), cuda)[:4]), c.eps)
    assert type(s.grad_fn).__name__ == type(y.grad_fn).__name__ == "_AddLayerNormBackward"


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_strided_arguments(cuda, op):
    """dy of stride 0 (y.sum().backward()) with, for the plain ops, x a transposed view (the op makes it contiguous)
    and, for the add ops, res a transposed view beside a contiguous x (the separate add and the plain norm).  All
    inside the bounds."""
    c = _mk(op, 6, 520)
    inp = _on(_inputs(c), cuda)
    ones = torch.ones_like(inp.gy)
    add = _is_add(op)
    base = (inp.x.clone() if add else inp.x.t().contiguous()).requires_grad_()
    w, b = inp.w.clone().requires_grad_(), None if inp.b is None else inp.b.clone().requires_grad_()
    rbase = inp.res.t().contiguous().requires_grad_() if add else None
    xv = base if add else base.t()                          # [d, rows] transposed: not contiguous
    assert add or not xv.is_contiguous()
    s, y = _apply(op, xv, rbase.t() if add else None, w, b, c.eps)
    if add:
        assert type(s.grad_fn).__name__ == "AddBackward0"
    saved = y.grad_fn.saved_tensors
    y.sum().backward()
    ref, bound, sref = _oracle(op, inp.x, inp.res, inp.w, inp.b, ones, None, c.eps)
    got = dict(y=y.detach(), rstd=saved[-1], mean=saved[-2], dx=base.grad if add else base.grad.t(), dw=w.grad,
               db=None if b is None else b.grad)
    r = _ratios(got, ref, bound)
    print(f"strided {op}: {_fmt(r)}")
    assert all(v <= 1.0 for v in r.values()), r
    if s is not None:
        assert torch.equal(s, sref) and _ratio(rbase.grad.t(), ref["dx"], bound["dx"]) <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["rms", "ln"])
def test_fp32_input_under_autocast(cuda, op):
    """fp32 x under bf16 autocast: taken as bf16(x), bf16 out, inside the bounds; the gradient returns as fp32."""
    c = _mk(op, 5, 520)
    inp = _on(_inputs(c), cuda)
    x32 = (inp.x.float() + 1e-3).requires_grad_()           # not bf16 values: the op rounds them
    w, b = inp.w.clone().requires_grad_(), None if inp.b is None else inp.b.clone().requires_grad_()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, y = _apply(op, x32, None, w, b, c.eps)
    assert y.dtype == torch.bfloat16
    y.backward(inp.gy)
    assert x32.grad.dtype == torch.float32
    ref, bound, _ = _oracle(op, x32.detach().to(torch.bfloat16), None, inp.w, inp.b, inp.gy, None, c.eps)
    got = dict(y=y.detach(), dx=x32.grad, dw=w.grad, db=None if b is None else b.grad)
    r = _ratios(got, ref, bound, [n for n in ("y", "dx", "dw", "db") if n in ref])
    assert all(v <= 1.0 for v in r.values()), r


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
def test_bf16_parameters_get_bf16_gradients(cuda, op):
    """bf16 weight / bias: the kernels run on their fp32 copies, the gradients are the fp32 results rounded once."""
    c = _mk(op, 37, 520)
    inp = _on(_inputs(c), cuda)
    wb, bb = inp.w.to(torch.bfloat16), None if inp.b is None else inp.b.to(torch.bfloat16)
    g32 = _run(op, inp._replace(w=wb.float(), b=None if bb is None else bb.float()), c.eps)
    g16 = _run(op, inp._replace(w=wb, b=bb), c.eps)
    assert g16["dw"].dtype == torch.bfloat16 and torch.equal(g16["dw"], g32["dw"].to(torch.bfloat16))
    if bb is not None:
        assert g16["db"].dtype == torch.bfloat16 and torch.equal(g16["db"], g32["db"].to(torch.bfloat16))
    assert torch.equal(g16["y"], g32["y"]) and torch.equal(g16["dx"], g32["dx"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", [_mk("rms", 4097, 64), _mk("add_rms", 4097, 64), _mk("ln", 4097, 1032),
                                  _mk("ln", 32771, 8), _mk("add_ln", 32771, 8)], ids=_id)
def test_same_call_twice_is_bitwise_equal(cuda, case):
    """Rows above every grid cap of the family: fixed summation orders, a last arriver that sums in split order."""
    inp = _data(case, cuda).inp
    one, two = _run(case.op, inp, case.eps), _run(case.op, inp, case.eps)
    for n in ("y", "dx", "dw", "db", "rstd", "mean"):
        if one.get(n) is not None:
            assert torch.equal(one[n], two[n]), n


# ------------------------------------------------------------------------------------------- GPU: direct ctypes calls
def _guarded(dev, n, dtype, pad=256):
    """n elements of ``dtype`` (bf16 or fp32) inside a buffer filled with the guard pattern, themselves guard-filled."""
    it, pat = (torch.int16, GUARD16) if dtype == torch.bfloat16 else (torch.int32, GUARD32)
    buf = torch.full((pad + n + pad,), pat, dtype=it, device=dev)
    return buf, buf[pad:pad + n].view(dtype)


def _guards_intact(buf, view, pad=256) -> bool:
    pat = GUARD16 if buf.dtype == torch.int16 else GUARD32
    return bool((buf[:pad] == pat).all()) and bool((buf[pad + view.numel():] == pat).all())


def _all_written(buf, view) -> bool:
    pat = GUARD16 if buf.dtype == torch.int16 else GUARD32
    return not bool((view.view(buf.dtype) == pat).any())


def _lib():
    from polyaxon_amd.ops import _native

    return _native.lib("plx_rms")


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _direct(c: Case, dev, lib, inp: Inputs):
    """Forward and backward of a case through the C entry points, every output inside guards.  Returns the outputs
    (dw / db summed from the partial rows in fp64) and the names of buffers whose guards broke or that kept a guard
    value inside."""
    op, rows, d = c.op, c.rows, c.d
    ln, add = _is_ln(op), _is_add(op)
    bf, f32 = torch.bfloat16, torch.float32
    st = _stream(dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    bufs = {}

    def out(name, n, dt):
        bufs[name] = _guarded(dev, n, dt)
        return bufs[name][1]

    y, rstd = out("y", rows * d, bf), out("rstd", rows, f32)
    s = out("s", rows * d, bf) if add else None
    mean = out("mean", rows, f32) if ln else None
    x, w = inp.x.contiguous(), inp.w.contiguous()
    if op == "rms":
        rc = lib.plx_rms_forward(p(x), p(w), p(y), p(rstd), rows, d, c.eps, st)
    elif op == "ln":
        rc = lib.plx_ln_forward(p(x), p(w), p(inp.b), p(y), p(mean), p(rstd), rows, d, c.eps, st)
    elif op == "add_rms":
        rc = lib.plx_add_rms_forward(p(x), p(inp.res), p(w), p(s), p(y), p(rstd), rows, d, c.eps, st)
    else:
        rc = lib.plx_add_ln_forward(p(x), p(inp.res), p(w), p(inp.b), p(s), p(y), p(mean), p(rstd), rows, d, c.eps, st)
    assert rc == 0
    nb = lib.plx_ln_bwd_blocks(rows, d) if ln else lib.plx_rms_bwd_blocks(rows)
    assert nb == _bwd_blocks(_path(op, d), rows)
    dx, pw = out("dx", rows * d, bf), out("dw_part", nb * d, f32)
    pb = out("db_part", nb * d, f32) if ln else None
    src = s if add else x
    if op == "rms":
        rc = lib.plx_rms_backward(p(src), p(w), p(inp.gy), p(rstd), p(dx), p(pw), rows, d, st)
    elif op == "ln":
        rc = lib.plx_ln_backward(p(src), p(w), p(inp.gy), p(mean), p(rstd), p(dx), p(pw), p(pb), rows, d, st)
    elif op == "add_rms":
        rc = lib.plx_add_rms_backward(p(src), p(w), p(inp.gy), p(rstd), p(inp.gs), p(dx), p(pw), rows, d, st)
    else:
        rc = lib.plx_add_ln_backward(p(src), p(w), p(inp.gy), p(mean), p(rstd), p(inp.gs), p(dx), p(pw), p(pb), rows,
                                     d, st)
    assert rc == 0
    torch.cuda.synchronize(dev)
    bad = [n for n, (b, v) in bufs.items() if not _guards_intact(b, v)]
    bad += [n + ":unwritten" for n, (b, v) in bufs.items() if not _all_written(b, v)]
    got = dict(y=y.view(rows, d), rstd=rstd, dx=dx.view(rows, d), dw=pw.view(nb, d).double().sum(0))
    if add:
        got.update(s=s.view(rows, d), dres=dx.view(rows, d))
    if ln:
        got.update(mean=mean, db=pb.view(nb, d).double().sum(0))
    return got, bad


@pytest.mark.gpu
@pytest.mark.parametrize("case", [_mk("rms", 5, 520), _mk("rms", 1030, 72), _mk("rms", 4099, 8), _mk("rms", 2, 8192),
                                  _mk("add_rms", 5, 2056), _mk("add_rms", 4099, 8), _mk("ln", 7, 520),
                                  _mk("ln", 4099, 8), _mk("ln", 3, 2056), _mk("ln", 1027, 1032), _mk("ln", 2, 8192),
                                  _mk("add_ln", 7, 1016), _mk("add_ln", 4099, 8), _mk("ln", 32771, 8)], ids=_id)
def test_direct_call_stays_inside_its_outputs(cuda, case):
    """Guard patterns before and after y, s, mean, rstd, dx and the partial matrices survive, every element between
    them is written, and the results (the partial rows summed in fp64) meet the bounds."""
    d = _data(case, cuda)
    got, bad = _direct(case, cuda, _lib(), d.inp)
    assert not bad, bad
    _check(case.op, got, d.ref, d.bound, d.s, f"{_id(case)} direct")


@pytest.mark.gpu
@pytest.mark.parametrize("d", [8, 64, 72, 8192])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1024, 2100])
def test_partial_colsum(cuda, rows, d):
    """plx_partial_colsum against an fp64 column sum, within gamma(chain) * sum |p| (+ the accumulate add): one and
    two matrices, store and accumulate independently per matrix, guards around the outputs, the level-2 workspace and
    the counters, counters back at zero, and a second launch on the same counters bitwise equal to the first."""
    lib = _lib()
    gen = torch.Generator().manual_seed(rows * 10007 + d)
    P = [torch.randn(rows, d, generator=gen).to(cuda) for _ in range(2)]
    O = [torch.randn(d, generator=gen).to(cuda) for _ in range(2)]
    st = _stream(cuda)
    ncol = (d + 63) // 64
    worst = 0.0
    for nz, acc in [(1, (0, 0)), (1, (1, 0)), (2, (0, 0)), (2, (1, 0)), (2, (0, 1)), (2, (1, 1))]:
        nws = int(lib.plx_partial_colsum_workspace(rows, d, nz))
        assert nws == nz * ((rows + 63) // 64) * d
        runs = []
        cbuf = torch.full((256 + nz * ncol + 256,), GUARD32, dtype=torch.int32, device=cuda)
        cnt = cbuf[256:256 + nz * ncol]
        cnt.zero_()
        for _ in range(2):
            wbuf, ws = _guarded(cuda, nws, torch.float32)
            outs = [_guarded(cuda, d, torch.float32) for _ in range(nz)]
            for z in range(nz):
                if acc[z]:
                    outs[z][1].copy_(O[z])
            o = [v for _, v in outs]
            rc = lib.plx_partial_colsum(P[0].data_ptr(), P[nz - 1].data_ptr(), rows, d, nz, ws.data_ptr(),
                                        cnt.data_ptr(), o[0].data_ptr(), o[nz - 1].data_ptr(), acc[0], acc[nz - 1], st)
            assert rc == 0
            torch.cuda.synchronize(cuda)
            assert _guards_intact(wbuf, ws) and _all_written(wbuf, ws)
            assert all(_guards_intact(b, v) and _all_written(b, v) for b, v in outs)
            assert bool((cnt == 0).all()) and bool((cbuf[:256] == GUARD32).all())
            assert bool((cbuf[256 + nz * ncol:] == GUARD32).all())
            runs.append([v.clone() for v in o])
        for z in range(nz):
            assert torch.equal(runs[0][z], runs[1][z]), (nz, acc, z)
            ref = P[z].double().sum(0) + (O[z].double() if acc[z] else 0.0)
            mag = P[z].double().abs().sum(0) + (O[z].double().abs() if acc[z] else 0.0)
            worst = max(worst, _ratio(runs[0][z], ref, _gamma(_colsum_depth(rows) + acc[z]) * mag))
    print(f"NORM_RATIO gpu colsum {rows}x{d}: colsum={worst:.3f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_argument_validation_launches_nothing(cuda):
    """Return code 1 for d % 8 != 0, d > 8192, rows <= 0 and nz outside 1..2, 2 for plx_add_ln_* above the wave
    path; nothing is launched, so guard-filled outputs stay guard-filled."""
    lib = _lib()
    rows, d = 4, 64
    st = _stream(cuda)
    bf = torch.zeros(rows * 8200, dtype=torch.bfloat16, device=cuda)
    f32 = torch.ones(8200, dtype=torch.float32, device=cuda)
    o16 = [torch.full((rows * 8200,), GUARD16, dtype=torch.int16, device=cuda) for _ in range(2)]
    o32 = [torch.full((rows * 8200,), GUARD32, dtype=torch.int32, device=cuda) for _ in range(4)]
    I, F, Y, S = bf.data_ptr(), f32.data_ptr(), o16[0].data_ptr(), o16[1].data_ptr()
    A, B, C, D = (t.data_ptr() for t in o32)
    for r, dd, want in ((rows, 100, 1), (rows, 8200, 1), (0, d, 1), (-3, d, 1), (rows, 4, 1)):
        assert lib.plx_rms_forward(I, F, Y, A, r, dd, 1e-5, st) == want
        assert lib.plx_rms_backward(I, F, I, F, Y, A, r, dd, st) == want
        assert lib.plx_add_rms_forward(I, I, F, S, Y, A, r, dd, 1e-5, st) == want
        assert lib.plx_add_rms_backward(I, F, I, F, I, Y, A, r, dd, st) == want
        assert lib.plx_ln_forward(I, F, F, Y, A, B, r, dd, 1e-5, st) == want
        assert lib.plx_ln_backward(I, F, I, F, F, Y, A, B, r, dd, st) == want
    for r, dd, want in ((rows, 100, 1), (0, d, 1), (-3, d, 1), (rows, 1032, 2), (rows, 2048, 2)):
        assert lib.plx_add_ln_forward(I, I, F, F, S, Y, A, B, r, dd, 1e-5, st) == want
        assert lib.plx_add_ln_backward(I, F, I, F, F, I, Y, A, B, r, dd, st) == want
    for r, dd, nz in ((0, d, 1), (-1, d, 2), (rows, 0, 1), (rows, d, 0), (rows, d, 3), (rows, d, -1)):
        assert lib.plx_partial_colsum(F, F, r, dd, nz, A, B, C, D, 0, 0, st) == 1
    torch.cuda.synchronize(cuda)
    assert all(bool((t == GUARD16).all()) for t in o16) and all(bool((t == GUARD32).all()) for t in o32)
