"""What the classifier's oracle tests share: the launch geometry of the scan restated (classifier_grid: checked against
csrc/classifier_grid.hpp over its whole range by tests/test_classifier_grid.py), the inputs whose scratch counters are not zero
(mixed_batch), and the CPU oracle's answers, computed once per batch and kept for every test of the session that needs them (oracle)."""
import numpy as np

from image_restoration_platform_amd import synth
from oracle import classifier as oc

CT_H, CT_W, CLS_MAX_WG, CLS_TICKET_CAP = 16, 256, 768, 64


def classifier_grid(n, h, w):
    """-> (tiles_x, tiles_y, per_img, rounds, tiles_of_last_workgroup) of a classifier launch of n images of h x w."""
    tx, ty = -(-w // CT_W), -(-h // CT_H)
    per = -(-(tx * ty) // -(-(tx * ty) // min(tx * ty, CLS_MAX_WG // n)))      # workgroup b walks tiles b, b + per, b + 2 per, ...
    return tx, ty, per, -(-(tx * ty) // per), (tx * ty) // per


KINDS = ("synth", "bytes", "binary_grey", "binary_rgb")


def mixed_batch(n, h, w, seed, first=0):
    """n images cycling through KINDS from KINDS[first]: synth.image (zero scratch counts: its gradients are far below the probes'
    threshold), uniform random bytes, random 0/255 with equal channels, random 0/255 with independent channels
    (the bottom right pixel of the 0/255 kinds is white)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, h, w, 3), np.uint8)
    for i in range(n):
        kind = KINDS[(first + i) % 4]
        if kind == "synth":
            out[i] = synth.image(seed + i, max(h, 8), max(w, 8))[:h, :w]
        elif kind == "bytes":
            out[i] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        elif kind == "binary_grey":
            out[i] = (rng.integers(0, 2, (h, w, 1), dtype=np.uint8) * 255)
        else:
            out[i] = rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255
        if kind.startswith("binary"):
            out[i, -1, -1] = 255          # the corner tile of a ragged image can be this one pixel: it must not be black
    return out


def tile_sums(img):
    """channel sum of every CT_H x CT_W tile of one image, [tiles_y, tiles_x]"""
    s = img.sum(axis=2, dtype=np.uint64)
    s = np.add.reduceat(s, np.arange(0, s.shape[0], CT_H), axis=0)
    return np.add.reduceat(s, np.arange(0, s.shape[1], CT_W), axis=1)


_ORACLE = {}


def oracle(key, imgs, is_jpeg):
    """The CPU oracle on every image of the batch -> [(scores, label, sums as a list of 14 ints)], computed once per `key` (the
    caller names the batch: the same key must mean the same pixels and flags).  Asserts the two conditions every such batch
    has to meet before an engine sees it: one image with all of sums[8..13] non-zero (the edge planes AND both scratch counters carry
    signal), and a non-zero channel sum in every tile of every image (a dropped or doubled tile must change sums[0..2])."""
    if key not in _ORACLE:
        jp = np.broadcast_to(np.asarray(is_jpeg, dtype=np.uint8), (len(imgs),))
        ref = []
        for i, im in enumerate(imgs):
            s, l, su = oc.classify(im, bool(jp[i]), with_sums=True)
            su = [int(x) for x in su.as_list()]
            t = tile_sums(im)
            assert int(t.sum()) == su[0] + su[1] + su[2], (key, i)         # the tiles add up to the oracle's own channel sums
            assert t.min() > 0, (key, i, "an all-black tile")
            ref.append((s, l, su))
        assert any(all(v > 0 for v in su[8:14]) for _, _, su in ref), (key, [su[8:14] for _, _, su in ref])
        _ORACLE[key] = ref
    return _ORACLE[key]


# The launches that reach the geometry classes of the scan which one-tile-per-workgroup shapes never do.  name -> (n, h, w, the first
# image's kind, classifier_grid(n, h, w) as the case was chosen: a change of the grid rule fails the case instead of moving it
# silently out of its class).
LAUNCHES = {
    "two_rounds_ragged": (8, 520, 600, 0, (3, 33, 50, 2, 1)),           # the smallest ragged two-round launch: workgroup 49 has one tile
    "benchmark": (8, 1024, 1024, 0, (4, 64, 86, 3, 2)),                 # bench.py's launch: three rounds, workgroups 84 and 85 take two tiles
    "batch32": (32, 392, 300, 0, (2, 25, 17, 3, 2)),                    # an engine with max_batch 32: 768 / 32 = 24 workgroups at most
    "batch64": (64, 200, 40, 0, (1, 13, 7, 2, 1)),                      # max_batch 64 = CLS_TICKET_CAP: 12 workgroups at most
    "second_pass_ragged": (1, 2090, 70, 2, (1, 131, 131, 1, 1)),        # 131 rows of `parts`: row lanes 0..2 of the finalize take a second step
    "parts_limit": (1, 6140, 300, 2, (2, 384, 768, 1, 1)),              # every row of `parts`, no tile loop
    "past_limit": (1, 6150, 300, 2, (2, 385, 385, 2, 2)),               # one tile row more: half the workgroups, two tiles each
    "second_pass_loop_batch": (3, 2400, 300, 1, (2, 150, 150, 2, 2)),   # finalize's second pass, the tile loop and a batch together
    "one_tile_each": (8, 16, 16, 1, (1, 1, 1, 1, 1)),                   # eight workgroups in all (between two big launches: stale `parts` rows)
}
_BATCHES = {}


def launch_batch(name):
    """-> (imgs [n, h, w, 3], is_jpeg [n] u8 with mixed flags, the oracle's answers), built once per session"""
    if name not in _BATCHES:
        n, h, w, first, _ = LAUNCHES[name]
        imgs = mixed_batch(n, h, w, seed=1000 + sorted(LAUNCHES).index(name), first=first)
        jp = (np.arange(n) % 3 != 1).astype(np.uint8)
        _BATCHES[name] = (imgs, jp, oracle(name, imgs, jp))
    return _BATCHES[name]
