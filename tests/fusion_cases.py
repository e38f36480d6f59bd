"""What the alignment tests of Fusion-v0 share (tests/test_fusion_cases.py on the CPU, tests/test_fusion_align_gpu.py on the GPU):
the oracle's alignment taken apart per view (decompose), the launch geometry of csrc/fusion.hip restated (geometry: its constants
are checked against the source text by test_fusion_cases.py), and the inputs -- planted shifts under which every one of the 81
coarse and 49 fine candidates has to win (COVER, COVER3), exactly periodic images whose candidates tie exactly (tie_cases), views
that share nothing (UNCORRELATED) and the smallest images that reach each launch shape (SHAPES).  Everything is plain numpy; the
oracle's answers are computed once per case and kept for every test of the session (reference)."""
import numpy as np

from image_restoration_platform_amd import synth
from oracle import fusion as ofu

CR, FR, FM = ofu.CR, ofu.FR, ofu.FM
NC, NF = (2 * CR + 1) ** 2, (2 * FR + 1) ** 2


def decompose(views):
    """-> per view v >= 1: (coarse winner (dy, dx), fine winner (dy, dx), coarse SAD table [9, 9], fine SAD table [7, 7]).
    oracle.fusion.align, restated with its own _sad_table / _pick (4 * coarse + fine == align(views)[v])."""
    L = [ofu.luma(v) for v in views]
    Q = [ofu.quarter(l) for l in L]
    out = []
    for v in range(1, len(views)):
        ct = ofu._sad_table(Q[0], Q[v], CR, CR, 1, 0, 0)
        c = ofu._pick(ct, CR)
        ft = ofu._sad_table(L[0], L[v], FR, FM, 2, 4 * c[0], 4 * c[1])
        out.append((c, ofu._pick(ft, FR), ct, ft))
    return out


# ---- the launch geometry (csrc/fusion.hip: SadCfg, FUSE_SAD_GRID, FUSE_FL, Engine::fuse_launch) -----------------------------------
TW = (128, 256)          # tile width in reference pixels, coarse / fine
SR = (8, 16)             # sampled reference rows per tile
SAD_GRID = 512           # workgroups per view at most
ROWSUM_PASS = 256 * 16   # elements of `part` one pass of the last workgroup's row sum takes (256 threads x FUSE_FL)
MAX_DIM, MAX_SETS = 8192, 16


def geometry(h, w, k=2, nsets=1, gcap=0):
    """The two SAD launches of one fuse call of `nsets` sets of k views of h x w; gcap > 0 = IRE_FUSE_GCAP.  Per search ("coarse",
    "fine"): tile columns and rows, the pixels of the last tile column, the sampled rows of the last tile row, workgroups per view
    G, tiles per workgroup at most, and the passes of the row sum over (k - 1) * G * N elements; for the coarse search also the
    quarter plane's pitch and the pixels in the interior's last dword (4 = full)."""
    cap = gcap if gcap > 0 else max(32, 512 // ((k - 1) * nsets))
    out = {}
    for mode, name in enumerate(("coarse", "fine")):
        ph, pw = (h // 4, w // 4) if mode == 0 else (h, w)
        m, step, n = (CR, 1, NC) if mode == 0 else (FM, 2, NF)
        iw, rows = pw - 2 * m, -(-(ph - 2 * m) // step)
        tx, ty = -(-iw // TW[mode]), -(-rows // SR[mode])
        g = min(SAD_GRID, cap, tx * ty)
        out[name] = dict(tiles_x=tx, tiles_y=ty, last_col_px=iw - (tx - 1) * TW[mode], last_row_rows=rows - (ty - 1) * SR[mode],
                         G=g, tiles_per_wg=-(-(tx * ty) // g), rowsum_passes=-(-((k - 1) * g * n) // ROWSUM_PASS))
    out["coarse"]["pitch"] = (w // 4 + 3) & ~3
    out["coarse"]["last_dword_px"] = (w // 4 - 2 * CR - 1) % 4 + 1
    return out


# ---- every candidate ---------------------------------------------------------------------------------------------------------------
COVER_H, COVER_W = 72, 88


def cover_seed(shift):
    return shift[0] * 100 + shift[1]


# Planted shifts (dy, dx) of view 1 at 72 x 88, views = synth.fusion_views(72, 88, shifts=((0, 0), s), seed=cover_seed(s)): a greedy
# cover of the grid dy, dx in [-19, 19] (every one of whose 1521 cases recovers its shift) under which the oracle's coarse winners are
# all 81 candidates and its fine winners all 49.  82 shifts: 81 is the least any cover can have.
COVER = [
    (0, 0), (-2, 0), (-1, -2), (-1, 2), (2, -1), (-2, -2), (-2, 3), (0, -6), (0, 6), (2, 4), (3, -3), (-7, 0), (7, 0), (-6, 2),
    (2, -6), (-3, -6), (-7, -3), (-3, 7), (3, 7), (0, -11), (0, 11), (9, 2), (10, 1), (-10, -3), (-14, 2), (-19, 0), (0, -19),
    (0, 19), (19, 0), (-19, -2), (-19, 2), (2, 19), (19, -2), (-3, -19), (-3, 19), (3, -19), (19, 3), (-6, -19), (19, 6), (-19, -7),
    (-19, 7), (7, 19), (19, -7), (9, -19), (-14, -19), (-14, 19), (19, -19), (19, 19), (7, -2), (-11, 0), (-6, -6), (-2, 10),
    (2, -10), (10, -2), (-7, 6), (-3, -10), (6, 7), (10, 3), (2, 12), (7, -7), (6, -10), (6, 10), (10, 6), (-11, 6), (-7, -10),
    (-6, 11), (-12, -6), (10, -8), (10, -10), (10, 10), (-7, 14), (6, -15), (-11, -11), (-11, 11), (-15, -10), (-15, 10), (10, 15),
    (14, -11), (-11, 15), (15, 11), (-15, -14), (-19, 19)]

# The k = 3 repack: set i plants COVER[i] in view 1 (same seed => the same pixels as the k = 2 case, so the same winners) and
# COVER3_VIEW2[i] in view 2.  View 2 has noise of its own, and a shift such as 6 = 4 * 1 + 2 = 4 * 2 - 2 has two decompositions, so its
# partners were searched for (greedily, with the oracle) until view 2's winners covered all 81 and all 49 as well.
COVER3_VIEW2 = [
    (-19, -19), (-19, -13), (-19, -8), (-19, -3), (-19, 2), (-19, 18), (-18, -1), (-18, 8), (-18, 10), (-14, -19), (-14, -6),
    (-14, -3), (-13, -13), (-13, -2), (-13, 4), (-13, 9), (-13, 18), (-12, 11), (-10, 19), (-8, -19), (-8, -12), (-8, -7), (-8, -2),
    (-8, -2), (-7, 2), (-7, 7), (-7, 12), (-5, -19), (-5, 19), (-3, -11), (-3, -6), (0, 19), (-2, -3), (-2, 4), (-2, -1), (1, -19),
    (5, 19), (-2, 10), (6, -19), (18, 2), (10, 19), (19, -19), (19, -13), (19, -8), (19, -3), (19, 6), (19, 6), (19, 19), (-19, 19),
    (-6, 6), (-2, -13), (-1, -10), (-2, -5), (-2, 12), (-2, 2), (-2, 7), (-1, -1), (2, -9), (2, -12), (2, -1), (2, 5), (2, 7),
    (2, 12), (3, -5), (6, -15), (6, 9), (6, -13), (6, -9), (6, -2), (6, -2), (6, 13), (6, 3), (10, -16), (10, -12), (10, -9),
    (11, -6), (10, -1), (10, 3), (10, 6), (10, 17), (10, 10), (15, 11)]


def cover_views(i, k=2):
    """the views of COVER[i] (k = 2) or of set i of the repack (k = 3), and the planted shifts [k, 2]"""
    shifts = ((0, 0), COVER[i]) + ((COVER3_VIEW2[i],) if k == 3 else ())
    return synth.fusion_views(COVER_H, COVER_W, shifts=shifts, seed=cover_seed(COVER[i])), np.array(shifts, np.int32)


def cover_batches():
    """-> [[indices into COVER]], at most 16 sets per batched call"""
    return [list(range(a, min(a + MAX_SETS, len(COVER)))) for a in range(0, len(COVER), MAX_SETS)]


# ---- exact ties ----------------------------------------------------------------------------------------------------------------------
def periodic(h, w, p):
    """grey image of period p on both axes (h % p == w % p == 0): a roll by any amount is the same image displaced, and candidates
    congruent mod p see equal pixels in every window (the margins keep the windows inside the plane) => exactly equal SADs.
    p = 4: the quarter plane is flat; p = 8: the quarter plane has period 2."""
    y, x = np.mgrid[0:h, 0:w]
    return ((x % p) * (120 // (p - 1)) + (y % p) * (75 // (p - 1)) + 30).astype(np.uint8)


def _rgb(*greys):
    return np.stack([np.repeat(g[..., None], 3, axis=2) for g in greys]).astype(np.uint8)


def _rolled(g, *rolls):
    return _rgb(g, *[np.roll(g, r, axis=(0, 1)) for r in rolls])


def _rows_x2(h, w):
    """period 2 in x only: every row has a level of its own (no structure in y)"""
    rows = np.random.default_rng(4242).integers(30, 200, h)
    return (rows[:, None] + (np.arange(w)[None, :] % 2) * 40).astype(np.uint8)


# name -> (views, per view v >= 1: the winning shift the case is named for, the table that decides it, the number of candidates at
# that table's minimum).  view_v = roll(view_0, r): its aligned sample view_v[y + dy, x + dx] equals view_0[y, x] for (dy, dx) = r mod p.
def tie_cases():
    h, w = COVER_H, COVER_W
    return {
        # fine minimum at the 16 candidates with dy and dx odd: Manhattan leaves (+-1, +-1), the (dy, dx) order picks (-1, -1)
        "p2_roll_1_1": (_rolled(periodic(h, w, 2), (1, 1)), [((-1, -1), "fine", 16)]),
        # flat quarter plane => coarse (0, 0); fine minimum at {-2, 2}^2, all of Manhattan 4: the order alone decides
        "p4_roll_2_2": (_rolled(periodic(h, w, 4), (2, 2)), [((-2, -2), "fine", 4)]),
        # the four candidates (1 mod 4, 1 mod 4) = {-3, 1}^2: Manhattan alone decides, against the order
        "p4_roll_1_1": (_rolled(periodic(h, w, 4), (1, 1)), [((1, 1), "fine", 4)]),
        # rows without structure pin dy (coarse 1, fine 0); the quarter plane is flat along x, and the fine dx ties among the odd values
        "p2_in_x_only": (_rolled(_rows_x2(h, w), (4, 1)), [((4, -1), "fine", 4)]),
        # the quarter plane has period 2 and is rolled by (1, 1): the COARSE search ties among its 16 odd candidates
        "p8_roll_4_4": (_rolled(periodic(h, w, 8), (4, 4)), [((-4, -4), "coarse", 16)]),
        # three views, a different tie per view: the second wave of the argmin and its own table
        "k3_p2_two_ties": (_rolled(periodic(h, w, 2), (1, 1), (0, 1)), [((-1, -1), "fine", 16), ((0, -1), "fine", 12)]),
        "k3_p4_two_ties": (_rolled(periodic(h, w, 4), (1, 1), (2, 2)), [((1, 1), "fine", 4), ((-2, -2), "fine", 4)]),
    }


# ---- small margins -------------------------------------------------------------------------------------------------------------------
# (seed, k, h, w): independent random bytes per view -- every candidate's SAD is within a few percent of every other's, so one that
# comes out too LOW wins where it must not.  Shapes with several tiles per search (SHAPES) and one single-tile shape; each shape once.
UNCORRELATED = [(301, 2, 64, 1064), (302, 3, 2048, 64), (303, 3, 64, 2048), (304, 2, 112, 64), (305, 3, 64, 72), (306, 2, 104, 64),
                (307, 3, 200, 328), (308, 2, 72, 88)]


def uncorrelated(seed, k, h, w):
    return np.random.default_rng(seed).integers(0, 256, (k, h, w, 3), dtype=np.uint8)


# ---- launch shapes -------------------------------------------------------------------------------------------------------------------
# name -> (h, w, planted shifts of views 1 and 2 (k = 2 takes the first), the properties the shape is there for as
# {(search, key of geometry(h, w, k=3)): value}).  The long axis carries a negative coarse shift, so that the view's staged rows /
# columns start before the reference's first tile.
SHAPES = {
    "rows63": (2048, 64, ((-14, 1), (9, -2)), {("coarse", "tiles_y"): 63, ("fine", "tiles_y"): 63, ("coarse", "rowsum_passes"): 3,
                                              ("fine", "rowsum_passes"): 2}),
    "cols4_8": (64, 2048, ((1, -14), (-2, 9)), {("coarse", "tiles_x"): 4, ("fine", "tiles_x"): 8, ("fine", "last_col_px"): 216}),
    "mask_in_col2": (64, 1064, ((1, -10), (-1, 7)), {("coarse", "tiles_x"): 3, ("coarse", "last_col_px"): 2,
                                                    ("coarse", "last_dword_px"): 2}),
    "max_w": (64, 8192, ((-1, -13), (2, 6)), {("coarse", "tiles_x"): 16, ("fine", "tiles_x"): 32}),
    "max_h": (8192, 64, ((-13, -1), (6, 2)), {("coarse", "tiles_y"): 255, ("fine", "tiles_y"): 255}),
    "pitch20": (64, 72, ((1, -6), (-2, 5)), {("coarse", "pitch"): 20, ("coarse", "last_col_px"): 10, ("coarse", "last_dword_px"): 2}),
    "fine_rows_2_full": (104, 64, ((-6, 1), (5, -2)), {("fine", "tiles_y"): 2, ("fine", "last_row_rows"): 16}),
    "fine_rows_partial": (112, 64, ((-6, 1), (5, -2)), {("fine", "tiles_y"): 3, ("fine", "last_row_rows"): 4}),
}


def shape_views(name, k):
    h, w, sh, _ = SHAPES[name]
    shifts = ((0, 0),) + tuple(sh[:k - 1])
    return synth.fusion_views(h, w, shifts=shifts, seed=900 + sorted(SHAPES).index(name))


# ---- IRE_FUSE_GCAP: what the child processes of test_workgroup_cap_walks_several_tiles_per_workgroup run ------------------------------
GCAP_SHAPES = [(2048, 64, ((-14, 1), (9, -2))), (64, 2048, ((1, -14), (-2, 9))), (200, 328, ((-7, 9), (11, -13)))]     # k = 3
GCAP_BATCH = (72, 1064)      # 16 sets of three views: 6 coarse tiles (the partial dword in the third column), 4 fine tiles


def gcap_batch():
    """-> (16 sets of three views of GCAP_BATCH with random shifts, their noise scores)"""
    rng = np.random.default_rng(8)
    sets, noise = [], []
    for i in range(MAX_SETS):
        sh = tuple((int(a), int(b)) for a, b in rng.integers(-19, 20, (2, 2)))
        sets.append(synth.fusion_views(*GCAP_BATCH, shifts=((0, 0),) + sh, seed=200 + i))
        noise.append(float(rng.uniform(0.0, 1.0)))
    return sets, noise


# ---- the oracle's answers, once per case ---------------------------------------------------------------------------------------------
_REF = {}


def reference(key, views, noise):
    """oracle.fusion.fuse(views, noise) -> (pixels, shifts), computed once per `key` (the same key must mean the same views and
    noise score); the arrays are shared: read only"""
    if key not in _REF:
        out, sh = ofu.fuse(views, noise)
        out.setflags(write=False)
        sh.setflags(write=False)
        _REF[key] = (out, sh)
    return _REF[key]
