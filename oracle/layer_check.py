"""Teacher-forced, per-element check of every RestoreNet layer -- TEST INFRASTRUCTURE ONLY.

For each captured layer the checker takes the INPUT tensor(s) of that layer as the engine stored them (bf16, exact in
float32), evaluates that ONE layer in float64, and compares with the engine's captured output of the same layer, element by
element.  No upstream rounding noise enters, so the bound is derived, not tuned.  Nothing here calls the engine or
oracle/restorenet.py: the layers are restated independently (GroupNorm -> FiLM -> SiLU -> round -> convolution, the composed
`up + fuse` weights, the fp8 operand rules).

The bound
---------
With `exact` the float64 value of an output element before its rounding, the engine's fp32 accumulator lies within

    b = (K + 2) * u * (|w| (*) |a| + |bias|)            fp32 accumulation of K products + bias in ANY order, u = 2^-24
      + |w| (*) (uncertain(a) * ulp(a))                   operand elements whose rounding may legitimately differ

of it ((*) = the same convolution on absolute values), and what the engine stores is a monotone function R of that accumulator
(one rounding to bf16; for a ResBlock's second convolution bf16(bf16(acc) + x): every kernel rounds the convolution BEFORE it adds
the residual, conv_rb / conv_pc / conv_pk / conv_w4 / conv_f8 / conv_mfma epilogues).  So the check is the interval

    R(exact - b) <= engine <= R(exact + b)

on every element: |engine - exact| <= 1/2 ulp_bf16 + b, stated without the flaw of that formula at a binade edge (an accumulator
that crosses a power of two rounds on the coarser grid) and with the residual layers' second rounding where it happens.  The
reported `bound` of an element is max(R(exact + b) - exact, exact - R(exact - b)).  All terms come from the reference; none from the
engine's output.  fp8 layers (weights e4m3 with one scale per output channel, the accumulator times that scale, accumulators
started at bias / scale): two more roundings, K + 4.

uncertain(a) and its window (the derived eps_act)
-------------------------------------------------
The activated operand a = round(silu(x A + B)) is recomputed here in float64 from the stored x and from the coefficients (A, B) the
kernel itself applied (captured with the layer as "<layer>.ab": floats, exact in float64); the engine computes it in fp32.  An element
is `uncertain` when its float64 pre-rounding value lies within 2 * delta of a rounding boundary of its format (bf16; fp8 engines: e4m3
of 16 silu -- the clamp at 448 is continuous and adds no boundary), delta being the sum of the documented error bounds of the engine's
sequence (conv_pk.hip's transform_group and the other producers: the same five steps), all absolute, u = 2^-24 (one fp32 rounding):

  y = x A + B  one fp32 fma, or a multiply and an add: u (|x A| + |y|) -- relative to |x A| + |B|, not to y.
  silu         t = y * fl(-log2 e): 1.25 u relative (product + constant); v_exp_f32 1 ulp = 2 u, its argument error |y| 1.25 u;
               1 + e: u; v_rcp_f32 1 ulp = 2 u; the final product u:
               |silu(y)| u (4 + (1 - sigma(y)) (2 + 1.25 |y|))   (instruction accuracies: AMD CDNA ISA guide, 1 ulp each)
               and |silu'(y)| dy for the error of y.
  delta = the sum; the window is TWICE that.

For |y| ~ 1 this is 2 * delta ~ 16 u = 2^-20 relative, i.e. ~5e-4 of the operand elements (measured on the engine: 1e-4 .. 1.5e-3).  The
helper asserts on every use that uncertain(a) covers at most 0.2 % of a layer's operand elements, that the median of bound /
ulp_bf16(exact) is at most 2, and it exempts no element.  Layers without an activation (stem, down, up, fuse) have no uncertain term.

The coefficients have a check of their own (check_coeffs): the captured (A, B) against the float64 GroupNorm + FiLM of the stored x,
within

  statistics   the GroupNorm partials are fp32 sums over the STORED bf16 values (fdot2_f32_bf16 on the packed output words in every
               producer's epilogue: conv_rb, conv_pc, conv_pk, conv_w4, conv_f8, conv_stem, conv_down, conv_dnq, conv_up, conv_upq,
               conv_mfma), one (sum, sum of squares) pair per tile and group, added up in double by gn_fold.hpp.  A tile's partial is a
               chain of at most 8 two-term fdot2 steps per thread followed by a lane tree (5 steps) and a merge over at most 16 waves:
               depth D <= 32, error <= D u sum|x| and D u sum x^2 (any summation of that depth).
               d_mean = D u mean|x|,  d_var = D u (mean x^2 + 2 |mean| mean|x|),  rstd: relative 1/2 d_var / (var + eps).
  coefficients gn_fold.hpp: mean and rstd rounded to float (u each), then float arithmetic
               rg = rstd g;  A = rg (1 + s);  B = (beta - mean rg)(1 + s) + t     one u per operation, propagated as written in
               _gn_coeffs; FiLM (s, t) = 7-term fp32 dot products + bias: 8 u (|cond| . |w| + |b|).

Why the coefficients are teacher-forced as well: the worst-case bound of the fp32 tile partials (D u, ~100 u on rstd where mean^2
exceeds the variance) is an order of magnitude wider than the SiLU sequence's; inside the operand window it made 2 % of the elements
uncertain on the reference alone.  Taking (A, B) from the engine keeps the window at the SiLU sequence's own error and still checks
the statistics, against the bound that belongs to them.

The partials-level check (coeffs_from_partials; tests/gn_cases.py, tests/test_gn_fold_gpu.py): gn_fold.hpp's reduction takes three
different paths per thread -- passes of its 8-chain unrolled loop, a tail loop, or no tile at all -- chosen by P, the partials per
image, and the shapes run() can afford stay below the P = 449 at which the first lane enters the unrolled loop.  So the standalone
finalize is also run on partials GIVEN to it (ire_debug_gn_finalize) at every pass structure, and judged against the same
coefficient formulas with what then remains of the statistics' bound: the partials are the input, so D = 0; gn_fold adds P
floats in double in a fixed order, in error by at most P 2^-53 sum|partial| / cnt on the mean and on the mean of squares (the bound of a
chain of P additions; gn_fold's tree is at most P / 512 + 21 deep, and from P = 26 on what it leaves unused covers the four double
operations between the sums and the variance -- two divisions, a square, a difference, 2^-53 relative each -- which have no term of
their own: the cases below that P are built so that all four are exact); mean and rstd rounded to float
and the float tail as above, one u per written operation (which covers a contracted fma: fewer roundings, not more).  An error of
one partial in P shifts a moment by 1 / P of it, ~2^-17 at the largest accepted image against a bound of ~2^-23: the tests' coded
partials are built so that no single dropped, repeated or misplaced partial stays inside it.  In the network, run_coeffs() applies
check_coeffs alone, with the moments taken in chunks from the captured float32 tensors, at shapes whose levels reach the unrolled
loop (1024 x 1024, 272 x 1000).

Final pixels: floor(clamp(in + y, 0, 255) + 0.5) is monotone in y as well; the two fp32 additions add u (|in + y| + 256) to b, and
the engine's pixel must lie in [pixel(exact - b), pixel(exact + b)]: equal to the reference except within b of a .5 boundary,
and there within 1 LSB.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
WIDTHS = (32, 64, 128, 256)
FILM_OFFSETS = (0, 64, 192, 448)
GN_EPS = 1e-5
STAT_DEPTH = 32                # depth of a tile partial's fp32 summation (docstring: statistics)
MAX_UNCERTAIN = 2e-3           # conditions asserted on every use
MAX_MEDIAN_ULPS = 2.0
TILE_H, TILE_W = 16, 32        # the producers' output tile at every level (engine.cpp kRbTileH x 32)
FP8_ACT_SCALE = 16.0
KEEP_ARRAYS = False             # tests of the checker itself: reports keep `exact` and `bound_ulps`


# ---------------------------------------------------------------------------------------------------------------------------
# number formats, exact in float64
# ---------------------------------------------------------------------------------------------------------------------------
def _ulp(v, mant_bits, min_exp):
    """Spacing of the format (mant_bits explicit mantissa bits, smallest normal 2^min_exp) in the binade of |v|."""
    _, e = np.frexp(np.abs(v))                                  # |v| = m 2^e, 0.5 <= m < 1
    e = np.maximum(e, min_exp + 1)
    return np.ldexp(1.0, e - 1 - mant_bits)


def bf16_ulp(v):
    return _ulp(v, 7, -126)


def bf16_round(v):
    """float64 -> nearest bf16 value (ties to even), as float64."""
    u = bf16_ulp(v)
    return np.rint(v / u) * u


def e4m3_ulp(v):
    return _ulp(v, 3, -6)


def e4m3_round(v):
    """float64 -> OCP e4m3fn (saturating at 448, ties to even, subnormals kept), as float64."""
    v = np.clip(v, -448.0, 448.0)
    u = e4m3_ulp(v)
    return np.rint(v / u) * u


def _boundary_distance(v, ulp):
    """Distance of v to the nearest rounding boundary (a midpoint of two neighbours) of the grid `ulp` of its binade."""
    r = np.abs(v) / ulp
    return (0.5 - np.abs(r - np.rint(r))) * ulp


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _nchw(a):          # captured NHWC -> NCHW float64
    return np.ascontiguousarray(np.transpose(np.asarray(a, dtype=np.float64), (0, 3, 1, 2)))


def _conv(x, w, stride=1, pad=1):
    with torch.no_grad():
        return F.conv2d(_t(x), _t(w), None, stride=stride, padding=pad).numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# GroupNorm -> FiLM -> SiLU -> round: the activated operand, its alternative roundings
# ---------------------------------------------------------------------------------------------------------------------------
def film_vectors(weights, scores):
    """(film, d_film): Linear(7 -> 960) of the scores as the engine holds them (double -> float), in float64, and the fp32 bound."""
    cond = np.asarray(scores, dtype=np.float64).astype(np.float32).astype(np.float64)
    w, b = weights["film.w"].astype(np.float64), weights["film.b"].astype(np.float64)
    return cond @ w.T + b[None, :], 8 * U * (np.abs(cond) @ np.abs(w).T + np.abs(b)[None, :])


def _gn_moments(x):
    """x [N,C,H,W] float64 -> per image and group (mean, mean|x|, mean x^2), each [N, 8]."""
    xg = x.reshape(x.shape[0], 8, -1)
    return xg.mean(axis=2), np.abs(xg).mean(axis=2), (xg * xg).mean(axis=2)


def _coeffs_from_moments(mean, mabs, msq, c, g, b, s, t, ds, dt, stat_depth=STAT_DEPTH, e_mean=None, e_msq=None):
    """Per-group moments [N, 8] of a tensor of c channels -> per-image, per-channel (A, B) of y = x A + B in float64 and their error
    bounds (dA, dB) for the engine's float path (module docstring: statistics, coefficients).  stat_depth: the depth of the fp32
    summation behind the moments the engine used (0: its partials are the given ones).  e_mean, e_msq [N, 8] (optional): a further
    absolute error of the engine's mean and mean x^2 (coeffs_from_partials: the double summation)."""
    var = np.maximum(msq - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + GN_EPS)
    d_mean = stat_depth * U * mabs + U * np.abs(mean)
    d_var = stat_depth * U * (msq + 2.0 * np.abs(mean) * mabs)
    if e_mean is not None:
        d_mean, d_var = d_mean + e_mean, d_var + e_msq + 2.0 * np.abs(mean) * e_mean
    e_rstd = 0.5 * d_var / (var + GN_EPS) + U                     # relative
    rep = c // 8
    mean, rstd, d_mean, e_rstd = (np.repeat(v, rep, axis=1) for v in (mean, rstd, d_mean, e_rstd))
    g, b = g.astype(np.float64)[None, :], b.astype(np.float64)[None, :]
    rg = rstd * g
    d_rg = np.abs(rg) * (e_rstd + U)
    p = 1.0 + s
    d_p = ds + U * np.abs(p)
    A = rg * p
    dA = d_rg * np.abs(p) + np.abs(rg) * d_p + U * np.abs(A)
    mrg = mean * rg
    d_mrg = d_mean * np.abs(rg) + np.abs(mean) * d_rg + U * np.abs(mrg)
    d = b - mrg
    d_d = d_mrg + U * np.abs(d)
    dp = d * p
    d_dp = d_d * np.abs(p) + np.abs(d) * d_p + U * np.abs(dp)
    B = dp + t
    dB = d_dp + dt + U * np.abs(B)
    return A, B, dA, dB


def _gn_coeffs(x, g, b, s, t, ds, dt):
    """x [N,C,H,W] float64 (stored bf16 values) -> (A, B, dA, dB) [N, C] of _coeffs_from_moments at the depth of the tile partials."""
    return _coeffs_from_moments(*_gn_moments(x), x.shape[1], g, b, s, t, ds, dt)


def partial_sums(stats, exact=False):
    """stats [N, P, 8, 2] float32 -> (sum, sum of absolute values) over the P partials, each [N, 8, 2] float64.  Summed image by image
    in float64 (exact for integer-valued partials below 2^53); exact=True: math.fsum, correctly rounded for any floats."""
    st = np.asarray(stats, dtype=np.float32)
    assert st.ndim == 4 and st.shape[2:] == (8, 2), st.shape
    tot, mag = np.zeros((st.shape[0], 8, 2)), np.zeros((st.shape[0], 8, 2))
    for i in range(st.shape[0]):
        v = st[i].astype(np.float64)
        if exact:
            import math
            for g in range(8):
                for k in range(2):
                    tot[i, g, k], mag[i, g, k] = math.fsum(v[:, g, k]), math.fsum(np.abs(v[:, g, k]))
        else:
            tot[i], mag[i] = v.sum(axis=0), np.abs(v).sum(axis=0)
    return tot, mag


def coeffs_from_sums(tot, mag, parts, hw, C, gamma, beta, s=None, t=None):
    """coeffs_from_partials behind the summation: tot, mag [N, 8, 2] as partial_sums returns them, parts = P."""
    n = tot.shape[0]
    assert tot.shape == mag.shape == (n, 8, 2) and C % 8 == 0
    cnt = float(hw) * (C // 8)
    e = parts * 2.0 ** -53 * mag / cnt
    zero = np.zeros((n, C))
    s, t = (zero if v is None else np.asarray(v, dtype=np.float32).astype(np.float64).reshape(n, C) for v in (s, t))
    return _coeffs_from_moments(tot[:, :, 0] / cnt, mag[:, :, 0] / cnt, tot[:, :, 1] / cnt, C, np.asarray(gamma), np.asarray(beta), s, t, zero, zero,
                                stat_depth=0, e_mean=e[:, :, 0], e_msq=e[:, :, 1])


def coeffs_from_partials(stats, hw, C, gamma, beta, s=None, t=None, exact=False):
    """(A, B, dA, dB) [N, C] of gn_fold.hpp on GIVEN partials: stats [N, P, 8, 2] float32 (sum, sum of squares per tile and group) of
    tensors of hw pixels and C channels, gamma / beta [C], the FiLM scale and shift s, t [N, C] as the floats the kernel reads (None: no
    FiLM).  The partials are summed in float64 (exact=True: math.fsum).  Nothing in front of the partials is judged, so
    stat_depth = 0 and no FiLM error; what remains of the statistics' bound is gn_fold's own summation, P terms in double in some
    order: at most P 2^-53 sum|partial| / cnt on the mean and on the mean of squares (module docstring: the partials-level check)."""
    tot, mag = partial_sums(stats, exact)
    return coeffs_from_sums(tot, mag, np.shape(stats)[1], hw, C, gamma, beta, s, t)


def reference_coeffs(x, weights, gn_prefix, level, film, d_film):
    """(A, B, dA, dB) [N, C] of the GroupNorm + FiLM in front of a convolution, from its stored input x."""
    c = x.shape[1]
    off = FILM_OFFSETS[level]
    s, t = film[:, off:off + c], film[:, off + c:off + 2 * c]
    ds, dt = d_film[:, off:off + c], d_film[:, off + c:off + 2 * c]
    return _gn_coeffs(x, weights[gn_prefix + ".g"], weights[gn_prefix + ".b"], s, t, ds, dt)


def check_coeffs(name, ab, ref):
    """The engine's captured (A, B) [N, C, 2] against the float64 coefficients within their derived bound -> '' or a message."""
    A, B, dA, dB = ref
    bad = ~((np.abs(ab[:, :, 0] - A) <= dA) & (np.abs(ab[:, :, 1] - B) <= dB))
    if not bad.any():
        return ""
    n, c = (int(v) for v in np.argwhere(bad)[0])
    return ("%s: GroupNorm+FiLM coefficients outside their bound for %d (image, channel) pairs; first: image %d channel %d (group %d): "
            "engine A %.9g B %.9g, exact A %.9g +- %.3g B %.9g +- %.3g"
            % (name, int(bad.sum()), n, c, c // (A.shape[1] // 8), ab[n, c, 0], ab[n, c, 1], A[n, c], dA[n, c], B[n, c], dB[n, c]))


def coeff_share(ab, ref):
    """Largest |engine - exact| / bound over all (image, channel) pairs and both coefficients (0 / 0 counts as 0): information."""
    A, B, dA, dB = ref
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.concatenate([(np.abs(ab[:, :, 0] - A) / dA).ravel(), (np.abs(ab[:, :, 1] - B) / dB).ravel()])
    return float(np.nan_to_num(r, nan=0.0, posinf=np.inf).max())


def activate(x, ab, fp8=False):
    """The activated MFMA operand of a convolution from its stored input x [N,C,H,W] and the coefficients ab [N,C,2] the engine applied
    (float, exact in float64): (a, step, info).
    a: the operand the reference multiplies (bf16, or e4m3 / 16 for fp8); step: 0 where the rounding is certain, else the distance to
    the neighbouring value the engine may legitimately hold instead."""
    A, B = ab[:, :, 0][:, :, None, None], ab[:, :, 1][:, :, None, None]
    xa = x * A
    y = xa + B
    dy = U * (np.abs(xa) + np.abs(y))
    with np.errstate(over="ignore"):
        sig = 1.0 / (1.0 + np.exp(-y))
    v = y * sig
    dsilu = np.abs(sig * (1.0 + y * (1.0 - sig))) * dy + np.abs(v) * U * (4.0 + (1.0 - sig) * (2.0 + 1.25 * np.abs(y)))
    dsilu = dsilu + 2.0 ** -126                                      # fp32 flush-to-zero of denormal intermediates
    if fp8:
        v, dsilu = v * FP8_ACT_SCALE, dsilu * FP8_ACT_SCALE
        a, ulp = e4m3_round(v), e4m3_ulp(np.minimum(np.abs(v) + 2 * dsilu, 448.0))
        dist = _boundary_distance(np.clip(v, -448.0, 448.0), e4m3_ulp(np.clip(v, -448.0, 448.0)))
        unc = (dist <= 2 * dsilu) & (np.abs(v) < 448.0)
        a, ulp = a / FP8_ACT_SCALE, ulp / FP8_ACT_SCALE
    else:
        a, ulp = bf16_round(v), bf16_ulp(np.abs(v) + 2 * dsilu)
        unc = _boundary_distance(v, bf16_ulp(v)) <= 2 * dsilu
    frac = float(unc.mean())
    assert np.isfinite(v).all(), "the activated operand is not finite"
    return a, np.where(unc, ulp, 0.0), {"uncertain": frac}


# ---------------------------------------------------------------------------------------------------------------------------
# weights as the engine holds them
# ---------------------------------------------------------------------------------------------------------------------------
def _wbf16(w):
    return bf16_round(np.asarray(w, dtype=np.float64))


def fp8_weights(w):
    """Per-output-channel e4m3 weights as weight_pack.hpp (pack_conv, fp8) states them: s_w = max|w[co]| / 448 (float),
    w_q = e4m3(w / s_w) (float division); -> (w_q * s_w in float64, K+4 roundings apply)."""
    w = np.asarray(w, dtype=np.float32)
    m = np.abs(w).reshape(w.shape[0], -1).max(axis=1)
    sw = np.where(m > 0, m / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    q = e4m3_round((w / sw[:, None, None, None]).astype(np.float32).astype(np.float64))
    return q * sw.astype(np.float64)[:, None, None, None]


_LO = ((0, 1), (0, 2))          # first / second window row of parity pa: taps ky = lo .. hi (conv_up.hip's sub-pixel pre-sums)
_HI = ((0, 2), (1, 2))


def subpixel_weights(w3, fp32_sum, rounded=True):
    """[co, ci, 3, 3] float64 -> [pa][pb] -> [co, ci, 2, 2]: nearest x2 -> 3x3 as four 2x2 convolutions on the low-res grid, the taps
    that land on one low-res pixel summed (fp32_sum: in float, as the plain `up` slabs; else in double and rounded to float as the
    composed ones), then ONE rounding to bf16."""
    out = [[None, None], [None, None]]
    for pa in range(2):
        for pb in range(2):
            k = np.zeros(w3.shape[:2] + (2, 2))
            for dy in range(2):
                for dx in range(2):
                    acc = np.zeros(w3.shape[:2], dtype=np.float32 if fp32_sum else np.float64)
                    for ky in range(_LO[pa][dy], _HI[pa][dy] + 1):
                        for kx in range(_LO[pb][dx], _HI[pb][dx] + 1):
                            acc = acc + w3[:, :, ky, kx].astype(acc.dtype)
                    k[:, :, dy, dx] = bf16_round(acc.astype(np.float32).astype(np.float64)) if rounded else acc
            out[pa][pb] = k
    return out


def _subpixel_conv(x, wsub):
    """x [N,Ci,h,w] -> [N,Co,2h,2w]: parity (pa, pb) output pixel (2y + pa, 2x + pb) reads low-res rows y - 1 + pa, y + pa."""
    n, _, h, w = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((n, wsub[0][0].shape[0], 2 * h, 2 * w))
    for pa in range(2):
        for pb in range(2):
            out[:, :, pa::2, pb::2] = _conv(xp[:, :, pa:pa + h + 1, pb:pb + w + 1], wsub[pa][pb], pad=0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# one layer: exact value, bound, verdict
# ---------------------------------------------------------------------------------------------------------------------------
class LayerReport:
    def __init__(self, name):
        self.name, self.ok, self.nfail, self.fails, self.message = name, True, 0, np.zeros((0, 4), int), ""
        self.headroom = self.median_ulps = self.uncertain = 0.0
        self.coeff_fail = False

    def __repr__(self):
        return "%s: %s headroom %.3f median bound %.2f ulp uncertain %.2e" % (self.name, "ok" if self.ok else "FAIL (%d)" % self.nfail,
                                                                             self.headroom, self.median_ulps, self.uncertain)


HEADROOM_GRID = (0.0, 0.125, 0.25, 0.5, 0.75, 1.0)


def _verdict(name, got, exact, center, b, R, unit, uncertain, level_note=""):
    """got / exact [N,C,H,W]; the engine stores R(accumulator), |accumulator - center| <= b; unit: ulp_bf16(exact) (1 for pixels).
    Every element is compared.  headroom: the largest share of b any element needs (smallest t of HEADROOM_GRID with
    R(center - t b) <= engine <= R(center + t b); inf if none): information, not a threshold."""
    rep = LayerReport(name)
    assert got.shape == exact.shape, (name, got.shape, exact.shape)
    assert np.isfinite(exact).all() and np.abs(exact).max() < 3.0e38, name + ": the float64 reference leaves the bf16 range"
    everything = (slice(None),) * got.ndim
    lo, hi = R(center - b, everything), R(center + b, everything)
    bound = np.maximum(hi - exact, exact - lo)
    ratio = np.zeros(got.shape)
    sel = np.nonzero(~(got == R(center, everything)))            # the grid only where the engine is not simply R(exact)
    if sel[0].size:
        g, c0, b0, need = got[sel], center[sel], b[sel], np.full(sel[0].size, np.inf)
        for t in HEADROOM_GRID[:0:-1]:
            need = np.where((g >= R(c0 - t * b0, sel)) & (g <= R(c0 + t * b0, sel)), t, need)
        ratio[sel] = need
    rep.uncertain = uncertain
    if KEEP_ARRAYS:
        rep.exact, rep.bound_ulps = exact, bound / unit
    rep.median_ulps = float(np.median(bound / unit))
    rep.headroom = float(ratio.max())
    assert uncertain <= MAX_UNCERTAIN, "%s: uncertain(a) covers %.3e of the operand (cap %.0e)" % (name, uncertain, MAX_UNCERTAIN)
    assert rep.median_ulps <= MAX_MEDIAN_ULPS, "%s: median bound %.2f ulp (cap %.0f)" % (name, rep.median_ulps, MAX_MEDIAN_ULPS)
    bad = ~((got >= lo) & (got <= hi))                      # (NaN fails)
    rep.nfail = int(bad.sum())
    if rep.nfail:
        rep.ok = False
        idx = np.argwhere(bad)                              # (n, c, y, x)
        rep.fails = idx[:, [0, 2, 3, 1]]                    # (n, y, x, c)
        worst = idx[np.argmax(np.where(np.isnan(ratio[bad]), np.inf, ratio[bad]))]
        n, c, y, x = (int(v) for v in worst)
        tiles = {}
        for i, _, yy, xx in idx:
            key = (int(i), int(yy) // TILE_H, int(xx) // TILE_W)
            tiles[key] = tiles.get(key, 0) + 1
        per_tile = ", ".join("img %d tile (%d,%d): %d" % (k + (v,)) for k, v in sorted(tiles.items())[:12])
        rep.message = ("%s%s: %d of %d elements outside the bound; worst at image %d (y %d, x %d, channel %d), tile (%d, %d) of %dx%d: "
                       "engine %.9g exact %.9g bound %.3g (allowed %.9g .. %.9g); failing elements per tile: %s%s"
                       % (name, level_note, rep.nfail, bad.size, n, y, x, c, y // TILE_H, x // TILE_W, TILE_H, TILE_W, got[n, c, y, x],
                          exact[n, c, y, x], bound[n, c, y, x], lo[n, c, y, x], hi[n, c, y, x], per_tile, " ..." if len(tiles) > 12 else ""))
    return rep


def _conv_layer(name, got, a, step, w, bias, uncertain, stride=1, pad=1, resid=None, extra_roundings=2, exact_add=None, bound_add=None):
    """exact = conv(a, w) + bias (+ exact_add); b as in the module docstring; engine = R(acc) (resid: bf16(bf16(acc) + resid))."""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    bias = np.asarray(bias, dtype=np.float64)[None, :, None, None]
    acc = _conv(a, w, stride, pad) + bias
    mag = _conv(np.abs(a), np.abs(w), stride, pad) + np.abs(bias)
    if exact_add is not None:
        acc, mag, K = acc + exact_add, mag + bound_add[0], K + bound_add[1]
    b = (K + extra_roundings) * U * mag
    if step is not None and uncertain > 0:
        b = b + _conv(step, np.abs(w), stride, pad)
    if resid is None:
        return _verdict(name, got, acc, acc, b, lambda v, sel: bf16_round(v), bf16_ulp(acc), uncertain)
    return _verdict(name, got, acc + resid, acc, b, lambda v, sel: bf16_round(bf16_round(v) + resid[sel]), bf16_ulp(acc + resid), uncertain)


def layer_inputs(name):
    """Names of the captured tensors a layer reads: (main input, second input or None).  'image' is the uint8 input."""
    def block_input(p):
        part, i = p.split(".rb")
        if i == "1":
            return part + ".rb0"
        if part == "enc0":
            return "stem"
        if part.startswith("enc"):
            return "down%d" % (int(part[3]) - 1)
        if part == "mid":
            return "enc3.rb1"
        return "fuse" + part[3]
    if name == "stem":
        return ("image", None)
    if name == "pixels":
        return ("dec0.rb1", "image")
    if name.startswith("down"):
        return ("enc%s.rb1" % name[4], None)
    if name.startswith("up") or name.startswith("fuse"):
        l = int(name[-1])
        return ("mid.rb1" if l == 2 else "dec%d.rb1" % (l + 1), "enc%d.rb1" % l)
    if name.endswith(".h"):
        return (block_input(name[:-2]), None)
    return (name + ".h", block_input(name))


def layer_names(up_mode="fused"):
    rb = lambda p: [p + ".h", p]
    names = ["stem"]
    for l in range(4):
        names += rb("enc%d.rb0" % l) + rb("enc%d.rb1" % l) + (["down%d" % l] if l < 3 else [])
    names += rb("mid.rb0") + rb("mid.rb1")
    for l in (2, 1, 0):
        names += ([] if up_mode == "fused" else ["up%d" % l]) + ["fuse%d" % l] + rb("dec%d.rb0" % l) + rb("dec%d.rb1" % l)
    return names + ["pixels"]


def gn_layer_names(up_mode="fused"):
    """The layers whose convolution applies a GroupNorm (their coefficients are captured as '<layer>.ab'; the head's as 'head.ab')."""
    return [nm for nm in layer_names(up_mode) if ".rb" in nm or nm == "pixels"]


def _level(name):
    if name in ("stem", "pixels"):
        return 0
    if name.startswith("mid"):
        return 3
    if name.startswith("down"):
        return int(name[4]) + 1
    return int(name[3]) if name[:3] in ("enc", "dec") else int(name[-1])


class NetworkCheck:
    """The checker for one call: images, scores and weights fixed; `get(name)` returns a captured tensor as NHWC float32
    (the engine's `activation(name).reshape(...)`, or the emulating oracle's capture).
    up_mode: 'fused' (default engine: up + fuse as one composed convolution, no `up` tensor), 'subpix' (IRE_UP_FUSE=0: sub-pixel `up`
    and a 1x1 `fuse`), 'plain' (IRE_UP_SUBPIX=0: nearest x2 + 3x3 and a 1x1)."""

    def __init__(self, weights, images, scores, get, pixels, fp8=False, up_mode="fused"):
        self.w = weights
        self.images = np.asarray(images)
        assert self.images.dtype == np.uint8 and self.images.ndim == 4
        self.film, self.d_film = film_vectors(weights, np.asarray(scores).reshape(self.images.shape[0], 7))
        self.get_raw, self.pixels, self.fp8, self.up_mode = get, np.asarray(pixels), fp8, up_mode
        assert up_mode in ("fused", "subpix", "plain")
        self._cache = {}
        self.chunk = 1 << 18                      # run_coeffs: elements per chunk of the float64 moments
        self.coeff_share = {}                     # run_coeffs: per layer the largest share of the coefficients' bound in use

    def get(self, name):
        if name == "image":
            return _nchw(self.images)
        if name not in self._cache:
            n, h, w, _ = self.images.shape
            l = _level(name)
            a = np.asarray(self.get_raw(name), dtype=np.float32)
            c = a.size // (n * (h >> l) * (w >> l))
            assert c * n * (h >> l) * (w >> l) == a.size, (name, a.size)
            a = _nchw(a.reshape(n, h >> l, w >> l, c))
            assert np.array_equal(bf16_round(a), a) or not np.isfinite(a).all(), name + ": captured values are not bf16"
            self._cache[name] = a
        return self._cache[name]

    def coeffs(self, name, gn_prefix, x, level):
        """The engine's captured coefficients of layer `name` [N, C, 2] float64, and '' or the message of their own check."""
        ab = np.asarray(self.get_raw(name + ".ab"), dtype=np.float32).astype(np.float64).reshape(x.shape[0], x.shape[1], 2)
        return ab, check_coeffs(name, ab, reference_coeffs(x, self.w, gn_prefix, level, self.film, self.d_film))

    def _rb_conv(self, name, prefix, conv, gn, x_in, resid):
        c = x_in.shape[1]
        f8 = self.fp8 and c >= 128
        ab, msg = self.coeffs(name, prefix + "." + gn, x_in, _level(name))
        a, step, info = activate(x_in, ab, fp8=f8)
        w = fp8_weights(self.w[prefix + "." + conv + ".w"]) if f8 else _wbf16(self.w[prefix + "." + conv + ".w"])
        rep = _conv_layer(name, self.get(name), a, step, w, self.w[prefix + "." + conv + ".b"], info["uncertain"], resid=resid,
                          extra_roundings=4 if f8 else 2)
        if msg:
            rep.ok, rep.coeff_fail, rep.message = False, True, (msg + "; " + rep.message if rep.message else msg)
        return rep

    def check(self, name):
        """-> LayerReport of one layer (every element compared)."""
        src, src2 = layer_inputs(name)
        if name == "stem":
            return _conv_layer(name, self.get(name), self.get("image"), None, _wbf16(self.w["stem.w"]), self.w["stem.b"], 0.0)
        if name == "pixels":
            return self._pixels()
        if name.startswith("down"):
            return _conv_layer(name, self.get(name), self.get(src), None, _wbf16(self.w[name + ".w"]), self.w[name + ".b"], 0.0, stride=2)
        if name.startswith("up"):
            x = self.get(src)
            w3 = _wbf16(self.w[name + ".w"])
            if self.up_mode == "plain":
                xu = np.repeat(np.repeat(x, 2, axis=2), 2, axis=3)
                return _conv_layer(name, self.get(name), xu, None, w3, self.w[name + ".b"], 0.0)
            return self._subpixel_layer(name, x, subpixel_weights(w3, True), self.w[name + ".b"], None, None)
        if name.startswith("fuse"):
            l = name[-1]
            wf = np.asarray(self.w[name + ".w"], dtype=np.float64)[:, :, 0, 0]            # [C, 2C]
            c = wf.shape[0]
            if self.up_mode != "fused":
                cat = np.concatenate([self.get("up" + l), self.get(src2)], axis=1)
                return _conv_layer(name, self.get(name), cat, None, _wbf16(wf)[:, :, None, None], self.w[name + ".b"], 0.0, pad=0)
            # weight_pack.hpp pack_up_fused: fuse(concat(up(x), skip)) = (Wf_up . Wup) * x_up + Wf_skip . skip + (Wf_up . b_up + b_f);
            # composition in double, sub-pixel pre-sums, ONE rounding to bf16; the bias in double, rounded to float
            wu, bu = np.asarray(self.w["up" + l + ".w"], dtype=np.float64), np.asarray(self.w["up" + l + ".b"], dtype=np.float64)
            wc = np.einsum("om,mikl->oikl", wf[:, :c], wu)
            bc = (np.asarray(self.w[name + ".b"], dtype=np.float64) + wf[:, :c] @ bu).astype(np.float32).astype(np.float64)
            return self._subpixel_layer(name, self.get(src), subpixel_weights(wc, False), bc, self.get(src2), _wbf16(wf[:, c:])[:, :, None, None])
        prefix = name[:-2] if name.endswith(".h") else name
        if name.endswith(".h"):
            return self._rb_conv(name, prefix, "conv1", "gn1", self.get(src), None)
        return self._rb_conv(name, prefix, "conv2", "gn2", self.get(src), self.get(src2))

    def _subpixel_layer(self, name, x, wsub, bias, skip, wskip):
        bias = np.asarray(bias, dtype=np.float64)[None, :, None, None]
        acc = _subpixel_conv(x, wsub) + bias
        mag = _subpixel_conv(np.abs(x), [[np.abs(k) for k in row] for row in wsub]) + np.abs(bias)
        K = 4 * x.shape[1]
        if skip is not None:
            acc, mag, K = acc + _conv(skip, wskip, pad=0), mag + _conv(np.abs(skip), np.abs(wskip), pad=0), K + skip.shape[1]
        b = (K + 2) * U * mag
        return _verdict(name, self.get(name), acc, acc, b, lambda v, sel: bf16_round(v), bf16_ulp(acc), 0.0)

    def _pixels(self):
        x = self.get("dec0.rb1")
        img = self.get("image")
        ab, msg = self.coeffs("head", "head.gn", x, 0)
        a, step, info = activate(x, ab)
        w = _wbf16(self.w["head.w"])
        bias = np.asarray(self.w["head.b"], dtype=np.float64)[None, :, None, None]
        y = _conv(a, w) + bias
        b = (w.shape[1] * 9 + 2) * U * (_conv(np.abs(a), np.abs(w)) + np.abs(bias)) + _conv(step, np.abs(w))
        b = b + U * (np.abs(img + y) + 256.0)                       # fl(in + y), fl(v + 0.5)
        every = (slice(None),) * 4
        pix = lambda v, sel=every: np.floor(np.clip(img[sel] + v, 0.0, 255.0) + 0.5)
        lo, hi = pix(y - b), pix(y + b)
        assert (hi - lo).max() <= 1.0, "pixels: the propagated bound spans more than one .5 boundary"
        rep = _verdict("pixels", _nchw(self.pixels), pix(y), y, b, pix, np.ones_like(y), info["uncertain"])
        rep.flips = float(np.mean(lo != hi))
        if msg:
            rep.ok, rep.coeff_fail, rep.message = False, True, (msg + "; " + rep.message if rep.message else msg)
        return rep

    def run(self, names=None):
        """-> {name: LayerReport} for the listed layers (default: all of this up_mode)."""
        return {nm: self.check(nm) for nm in (names or layer_names(self.up_mode))}

    def _chunked_moments(self, src, level, chunk=None):
        """(mean, mean|x|, mean x^2) [N, 8] and C of the captured tensor `src`, straight from its float32 NHWC array in chunks of about
        `chunk` elements (cache-sized: the walk is bound by memory) into float64 accumulators; no float64 copy of the tensor is made or kept.  The products of bf16 values are exact
        in float64; a sum of N terms in any order is within N 2^-53 of sum|x| relative (N <= 2^22 per group here: 2^-31, against a
        bound of STAT_DEPTH 2^-24)."""
        n, h, w, _ = self.images.shape
        h, w = h >> level, w >> level
        a = np.asarray(self.get_raw(src), dtype=np.float32)
        c = a.size // (n * h * w)
        assert c % 8 == 0 and c * n * h * w == a.size, (src, a.size)
        a = a.reshape(n, h * w, c)
        acc = np.zeros((3, n, c))                                    # per channel; the channels of a group are added last
        step = max(1, (chunk or self.chunk) // c)
        for i in range(n):
            for r in range(0, h * w, step):
                v = a[i, r:r + step].astype(np.float64)
                acc[0, i] += v.sum(axis=0)
                acc[2, i] += np.einsum("pc,pc->c", v, v)
                acc[1, i] += np.abs(v, out=v).sum(axis=0)
        acc = acc.reshape(3, n, 8, c // 8).sum(axis=3)
        return acc[0] / (h * w * (c // 8)), acc[1] / (h * w * (c // 8)), acc[2] / (h * w * (c // 8)), c

    def run_coeffs(self, names=None):
        """The coefficients alone: for every listed layer that applies a GroupNorm (default: all of them; `pixels` is the head, captured
        as head.ab) the captured (A, B) against the float64 GroupNorm + FiLM of the captured input, within check_coeffs' bound ->
        {name: '' or the message}.  No convolution is evaluated and no tensor is converted whole, so the walk is affordable at shapes
        where run() is not (1024 x 1024: tens of thousands of tiles per image for gn_fold.hpp to add up)."""
        out = {}
        for nm in (names or gn_layer_names(self.up_mode)):
            assert nm == "pixels" or ".rb" in nm, nm + ": no GroupNorm in front of this layer"
            prefix = nm[:-2] if nm.endswith(".h") else nm
            gn = "head.gn" if nm == "pixels" else prefix + (".gn1" if nm.endswith(".h") else ".gn2")
            level = _level(nm)
            mean, mabs, msq, c = self._chunked_moments(layer_inputs(nm)[0], level)
            off = FILM_OFFSETS[level]
            ref = _coeffs_from_moments(mean, mabs, msq, c, self.w[gn + ".g"], self.w[gn + ".b"], self.film[:, off:off + c], self.film[:, off + c:off + 2 * c],
                                       self.d_film[:, off:off + c], self.d_film[:, off + c:off + 2 * c])
            ab = np.asarray(self.get_raw(("head" if nm == "pixels" else nm) + ".ab"), dtype=np.float32).astype(np.float64).reshape(mean.shape[0], c, 2)
            out[nm] = check_coeffs("head" if nm == "pixels" else nm, ab, ref)
            self.coeff_share[nm] = coeff_share(ab, ref)
        return out


def assert_network(weights, images, scores, get, pixels, fp8=False, up_mode="fused", names=None, label=""):
    """Check every layer; raise one AssertionError naming every failing layer (layer, image, pixel, tile, values).  -> reports."""
    reports = NetworkCheck(weights, images, scores, get, pixels, fp8=fp8, up_mode=up_mode).run(names)
    bad = [r.message for r in reports.values() if not r.ok]
    assert not bad, "%s%d layer(s) outside the derived bound:\n  %s" % (label and label + ": ", len(bad), "\n  ".join(bad))
    return reports


def stress_weights(w0):
    """A hand-made weight set derived from another (the tests use seed 0) that walks the layers' edges: FiLM rows scaled and some
    scale biases at -2.5 (1 + s negative), GroupNorm gains of both signs with a few exact zeros, biases of 4.0 on every fourth channel
    of one convolution per level (outputs in the coarse bf16 ulps; on EVERY channel the next GroupNorm's x A and B cancel from ~4 rstd
    and the uncertain set exceeds its cap on the reference alone: tamed), one ResBlock convolution with all-zero weights (its output is its bias: the GroupNorm
    behind it sees groups of variance ~4e-4, rstd ~ 50).  A constant bias there (variance exactly 0, rstd = 1 / sqrt(eps)) was tried
    and tamed: x A and B then cancel from ~80 to ~0.1 in fp32 and the uncertain set exceeds its 0.2 % cap on the reference alone."""
    w = {k: np.array(v, dtype=np.float32, copy=True) for k, v in w0.items()}
    for l, c in enumerate(WIDTHS):
        off = FILM_OFFSETS[l]
        w["film.w"][off:off + c] *= 8.0
        w["film.b"][off:off + c:5] = -2.5
    for k in w:
        if k.endswith(".g"):
            w[k][1::3] *= -1.0
            w[k][::11] = 0.0
    for l in range(4):
        w["enc%d.rb0.conv1.b" % l][::4] = 4.0
    w["dec1.rb0.conv1.w"][:] = 0.0
    return w


FP8_CLAMP_LAYERS = {"enc2.rb1": "enc2.rb1.gn2", "enc3.rb0.h": "enc3.rb0.gn1", "mid.rb0.h": "mid.rb0.gn1", "dec2.rb0": "dec2.rb0.gn2"}
FP8_ZERO_ROW_CONV = "mid.rb1.conv1"


def fp8_stress_weights(w0):
    """stress_weights(w0) with the two edges of the fp8 operand rules on top, which neither the seeds nor the stress set reach (with
    them the largest 16 silu(x A + B) at a C >= 128 layer is 325):
    (a) the GroupNorm gains of channels 2::7 times 12 in front of the four convolutions of FP8_CLAMP_LAYERS (conv1 and conv2, with and
        without the residual, C = 128 and C = 256): a share of 4e-3 .. 1e-2 of their activated operands has 16 silu >= 448, the largest
        1024 .. 2337, so the clamp in front of the e4m3 conversion decides what the MFMA multiplies;
    (b) the output rows ::9 of FP8_ZERO_ROW_CONV all zero: max|w| == 0, the scale 1.0 of fp8_weights and weight_pack.hpp::pack_conv;
        those channels' output is their bias.
    (b) was run on the CPU at 72 x 136 with the three stress images as written, and nothing had to be tamed: 29 of the 256 channels
    of mid.rb1.h are constant per image, at most four of the 32 in a GroupNorm group, so no group's variance collapses (the constant
    bias that stress_weights' docstring tames is the case of EVERY channel of a group); every layer of the intact fp8 oracle passes
    and the caps hold (tests/test_layer_check.py asserts it, and prints the shares)."""
    w = stress_weights(w0)
    for gn in FP8_CLAMP_LAYERS.values():
        w[gn + ".g"][2::7] *= 12.0
    w[FP8_ZERO_ROW_CONV + ".w"][::9] = 0.0
    return w


def clamp_share(x, ab):
    """Share of the activated fp8 operands of a convolution (stored input x [N,C,H,W], applied coefficients ab [N,C,2]) with
    16 silu(x A + B) >= 448, and the largest 16 silu: what the clamp in front of the e4m3 conversion acts on."""
    y = x * ab[:, :, 0][:, :, None, None] + ab[:, :, 1][:, :, None, None]
    with np.errstate(over="ignore"):
        v = FP8_ACT_SCALE * y / (1.0 + np.exp(-y))
    return float((v >= 448.0).mean()), float(v.max())
