"""GroupNorm partials for csrc/gn_fold.hpp at every pass structure of its reduction -- shared by tests/test_gn_cases.py (the CPU
proof that the cases can see a defect) and tests/test_gn_fold_gpu.py (the kernel on them).

gn_fold runs with 512 threads: 64 tile lanes (tl = tid >> 3) x 8 groups.  Lane tl starts at tile t = tl and takes
  full passes   while t + 7 * 64 < P: tiles t, t + 64, .., t + 448 into eight chains, t += 512;
  tail steps    while t < P: tile t into chain 0, t += 64                          (0 .. 7 of them);
  nothing       when tl >= P.
regimes(P) restates those two loops and nothing else.

Coded partials: exact small integers, so the moments are exact in float64 and on the device, and the only error left is the float
tail's.  With B = ceil(log2 P), image b < B carries in group g of tile t
    sum = 2048 bit[(b + g) mod B](t),    sumsq = 2048 (1 + 3 bit[(b + g + 5) mod B](t)) + 128 b,
(the term 128 b tells the images apart: where P is a power of two every bit is set in half of the tiles and the coded images would
otherwise share all their moments, so that one image's partials read for another's could not show),
so every bit of t reaches every group's mean in some image and its mean of squares in some image: a tile that is dropped, read in
another's place or taken from another tile's address moves a moment of some image by 1 / P (hw (C / 8) = 2048 P: one tile is one
2048-element share).  A last image has sum = 2048 and sumsq = 2048 (g + 1) everywhere: the groups differ in EVERY tile, which the
all-zero and all-one tile indices of the coded images cannot offer."""
import functools

import numpy as np

NTL = 64                      # tile lanes of gn_fold's 512 threads
WEIGHT = 2048.0               # elements per tile and group, and the unit of the coded partials
IMAGE_TAG = 128.0             # per image index and tile on the sums of squares: 1 / 16 of a unit on the mean of squares

SWEEP = (1, 8, 63, 64, 65, 448, 449, 450, 511, 512, 513, 544, 960, 1023, 1024, 1025, 2048, 8192, 131072)
WIDTHS = (32, 64, 128, 256)


def lane_regimes(P):
    """[(full passes, tail steps)] of the 64 tile lanes, by running gn_fold's two loop headers."""
    out = []
    for tl in range(NTL):
        t, full, tail = tl, 0, 0
        while t + 7 * NTL < P:
            t += 8 * NTL
            full += 1
        while t < P:
            t += NTL
            tail += 1
        out.append((full, tail))
    return out


def regimes(P):
    """((min, max) full passes, (min, max) tail steps) over the 64 tile lanes."""
    lanes = lane_regimes(P)
    return ((min(f for f, _ in lanes), max(f for f, _ in lanes)), (min(t for _, t in lanes), max(t for _, t in lanes)))


# every structurally different mix of lanes; test_gn_cases asserts that SWEEP holds a P of each
CLASSES = {
    "idle lanes": lambda l: (0, 0) in l,
    "one tail step on every lane, no pass": lambda l: set(l) == {(0, 1)},
    "tail only, lanes differ by a step": lambda l: all(f == 0 for f, _ in l) and len({t for _, t in l}) == 2 and (0, 0) not in l,
    "7 tail steps on every lane, no pass": lambda l: set(l) == {(0, 7)},
    "some lanes one pass, the others 7 tail steps": lambda l: set(l) == {(1, 0), (0, 7)},
    "one clean pass": lambda l: set(l) == {(1, 0)},
    "a pass, then a tail step on some lanes": lambda l: set(l) == {(1, 0), (1, 1)},
    "a pass, then 7 tail steps on every lane": lambda l: set(l) == {(1, 7)},
    "lanes with one pass and lanes with two": lambda l: {f for f, _ in l} == {1, 2},
    "clean passes, several": lambda l: len(set(l)) == 1 and l[0][0] >= 2 and l[0][1] == 0,
    "several passes, then a tail step on some lanes": lambda l: set(l) == {(2, 0), (2, 1)},
    "256 passes (the largest accepted image)": lambda l: set(l) == {(256, 0)},
}


def hw_for(P, C):
    """Pixels per image with hw (C / 8) = 2048 P."""
    return int(WEIGHT) * P * 8 // C


@functools.lru_cache(maxsize=1)
def coded_partials(P):
    """[B + 1, P, 8, 2] float32 (read-only): the coded images and the image of constant tiles."""
    B = (P - 1).bit_length()                      # ceil(log2 P)
    t = np.arange(P, dtype=np.int64)
    st = np.empty((B + 1, P, 8, 2), np.float32)
    for b in range(B):
        for g in range(8):
            st[b, :, g, 0] = WEIGHT * ((t >> ((b + g) % B)) & 1)
            st[b, :, g, 1] = WEIGHT * (1 + 3 * ((t >> ((b + g + 5) % B)) & 1)) + IMAGE_TAG * b
    st[B, :, :, 0] = WEIGHT
    st[B, :, :, 1] = WEIGHT * np.arange(1, 9, dtype=np.float32)[None, :]
    st.setflags(write=False)
    return st


def coded_gamma_beta(C):
    """Gains of both signs in 0.5 .. 1.5 and offsets in -1.25 .. 1.25, exact in float."""
    c = np.arange(C)
    gamma = (0.5 + (c * 7 % 17) / 16.0) * np.where(c % 3 == 1, -1.0, 1.0)
    beta = (c * 5 % 11 - 5) / 4.0
    return gamma.astype(np.float32), beta.astype(np.float32)


# ---- float cases ----------------------------------------------------------------------------------------------------------
def _plausible(rng, nimg, P, per_tile):
    """Partials as a producer writes them: per tile and group `per_tile` values of mean mu_g, deviation sd_g."""
    mu, sd = rng.uniform(-2.0, 2.0, (nimg, 1, 8)), rng.uniform(0.05, 3.0, (nimg, 1, 8))
    m = mu + sd * rng.standard_normal((nimg, P, 8)) / np.sqrt(per_tile)
    v = sd * sd * (1.0 + 0.1 * rng.standard_normal((nimg, P, 8)))
    return np.stack([per_tile * m, per_tile * (np.abs(v) + m * m)], axis=-1).astype(np.float32)


def _film(rng, nimg, C, stride, off, lo=-0.6, hi=0.6):
    f = rng.uniform(-9.0, 9.0, (nimg, stride)).astype(np.float32)        # what lies around the window must not matter
    f[:, off:off + C] = rng.uniform(lo, hi, (nimg, C))
    f[:, off + C:off + 2 * C] = rng.uniform(-1.0, 1.0, (nimg, C))
    return f


def float_cases():
    """[dict(name, stats, hw, C, gamma, beta, film, film_off)], seeded.  film None: no FiLM."""
    cases = []

    def add(name, stats, hw, C, gamma=None, beta=None, film=None, film_off=0, seed=0):
        rng = np.random.default_rng(1000 + seed)
        gamma = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C) if gamma is None else gamma
        beta = rng.uniform(-1.0, 1.0, C) if beta is None else beta
        cases.append(dict(name=name, stats=np.ascontiguousarray(stats, dtype=np.float32), hw=int(hw), C=C, gamma=np.asarray(gamma, np.float32),
                          beta=np.asarray(beta, np.float32), film=film, film_off=film_off))

    # partials of mixed sign and magnitude 1e-3 .. 1e4 (sums cancel; the sums of squares stay positive)
    rng = np.random.default_rng(1)
    P, C = 1023, 64
    s = 10.0 ** rng.uniform(-3, 4, (3, P, 8)) * rng.choice([-1.0, 1.0], (3, P, 8))
    q = 10.0 ** rng.uniform(-3, 4, (3, P, 8))
    add("mixed sign and magnitude", np.stack([s, q], -1), 512 * P // 8, C, film=_film(rng, 3, C, 2 * C, 0), seed=1)

    # every tile equal, mean m and mean of squares m^2 exact: variance exactly 0, rstd = 1 / sqrt(1e-5)
    m = np.array([0.0, 0.25, -1.5, 3.0, 1.0, -0.125, 2.5, -4.0])
    eq = np.broadcast_to(np.stack([WEIGHT * m, WEIGHT * m * m], -1)[None, None], (2, 544, 8, 2)).astype(np.float32)
    rng = np.random.default_rng(2)
    add("variance exactly 0", eq, hw_for(544, 128), 128, film=_film(rng, 2, 128, 2 * 128, 0), seed=2)

    # the same with every sum of squares one float below m^2's: sumsq / cnt - mean^2 < 0, clamped at 0
    neg = eq.copy()
    neg[..., 1] = np.nextafter(neg[..., 1], np.float32(0.0))
    add("variance slightly negative", neg, hw_for(544, 128), 128, seed=3)

    # hw G no power of two (and no multiple of P): the divisions by cnt round
    rng = np.random.default_rng(4)
    add("hw G not a power of two", _plausible(rng, 3, 450, 583.1), 200 * 328 - 1, 32, film=_film(rng, 3, 32, 64, 0), seed=4)

    # gains of both signs with exact zeros
    rng = np.random.default_rng(5)
    g = rng.uniform(0.2, 2.0, 256) * rng.choice([-1.0, 1.0], 256)
    g[::5] = 0.0
    add("gamma of both signs with zeros", _plausible(rng, 2, 513, 512.0), 513 * 512 // 32, 256, gamma=g, film=_film(rng, 2, 256, 512, 0), seed=5)

    # 1 + s = 0 and below
    rng = np.random.default_rng(6)
    f = _film(rng, 3, 64, 128, 0)
    f[:, 0:64:3] = -1.0
    f[:, 1:64:3] = -2.5
    add("FiLM scale at -1 and below", _plausible(rng, 3, 960, 512.0), 960 * 512 // 8, 64, film=f, seed=6)

    # a window inside a longer row
    rng = np.random.default_rng(7)
    add("film window off 13 in rows of 2 C + 37", _plausible(rng, 4, 449, 512.0), 449 * 512 // 4, 32, film=_film(rng, 4, 32, 2 * 32 + 37, 13), film_off=13, seed=7)

    # no FiLM
    rng = np.random.default_rng(8)
    add("no film", _plausible(rng, 2, 2048, 512.0), 2048 * 512 // 16, 128, seed=8)
    return cases


def case_reference(lc, case):
    """(A, B, dA, dB) of a float case: oracle.layer_check.coeffs_from_partials with the sums taken by math.fsum."""
    C, off, film = case["C"], case["film_off"], case["film"]
    s, t = (None, None) if film is None else (film[:, off:off + C], film[:, off + C:off + 2 * C])
    return lc.coeffs_from_partials(case["stats"], case["hw"], C, case["gamma"], case["beta"], s, t, exact=True)


def many_images_case(nimg=64, P=513, C=64):
    """One call, nimg images of different content (the kernel's image index is its workgroup index)."""
    rng = np.random.default_rng(64)
    return dict(name="%d images" % nimg, stats=_plausible(rng, nimg, P, 512.0), hw=P * 512 * 8 // C, C=C,
                gamma=rng.uniform(-1.5, 1.5, C).astype(np.float32), beta=rng.uniform(-1.0, 1.0, C).astype(np.float32),
                film=_film(rng, nimg, C, 2 * C + 3, 2), film_off=2)
