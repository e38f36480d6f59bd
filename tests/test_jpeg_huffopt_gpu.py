"""JPEG results with optimised Huffman tables on the device (csrc/jpeg.hip: count pass, table kernel, emit pass) against the model
(tests/jpeg_huffopt_model.py, which tests/test_jpeg_huffopt_model.py holds to libjpeg-turbo's file): every pixel case through the
host entry, the windowed device entry and the tensor entry; tables that do not leak between the images of one call; the table
kernel alone on the native test's histograms; every job kind on engines created with IRE_FLAG_JPEG_OPTIMIZE; the same decoded pixels
as the fixed-table file; and the fixed-table path untouched."""
import base64
import ctypes
import functools
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_huffopt_cases as cases      # noqa: E402
import jpeg_huffopt_model as model      # noqa: E402
import jpeg_opt_model as opt            # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def want_text(name, q, s):
    return model.jpeg_base64(cases.image(name), q, s)


def _decode(text, h, w):
    """Pillow reads the file without a warning, to the declared size"""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(base64.b64decode(text)))
        im.load()
        assert im.format == "JPEG" and im.mode == "RGB" and im.size == (w, h)
        return np.asarray(im)


def _first_difference(got, want):
    try:
        a, b = base64.b64decode(got + b"=" * (-len(got) % 4)), base64.b64decode(want)
    except Exception:
        return None
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def _same(got, want, what):
    if got != want:
        pytest.fail("%s: %d characters where the model has %d; first differing file byte %s" % (what, len(got), len(want), _first_difference(got, want)))


def _window(px):
    """[n][h][w][3] on the host -> the same pixels as a window of a larger device tensor: rows and images apart"""
    import torch
    n, h, w, _ = px.shape
    big = torch.full((n, h + 5, w + (7 if w % 2 == 0 else 6), 3), 0x3C, dtype=torch.uint8, device="cuda")
    big[:, :h, :w] = torch.from_numpy(px).cuda()
    t = big[:, :h, :w]
    assert t.stride(1) % 2 == 1 and t.stride(1) > 3 * w and t.stride(0) > h * t.stride(1)
    return t


def _device_entry(eng, t, q, s, surplus=517):
    """ire_encode_jpeg_optimized_base64_fit_device of the view t into guard-filled texts -> (texts, lens) on the host"""
    import torch
    n, h, w, _ = t.shape
    stride = eng.jpeg_base64_bound(h, w, q, s, optimize=True) + surplus
    out = torch.full((n, stride), GUARD, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = eng._lib.ire_encode_jpeg_optimized_base64_fit_device(eng._h, ctypes.c_void_p(t.data_ptr()), n, h, w, t.stride(1), t.stride(0), ctypes.c_void_p(out.data_ptr()), stride,
                                                              ctypes.c_void_p(lens.data_ptr()), q, s, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.IRE_OK, eng._lib.ire_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy()


@pytest.mark.parametrize("name", cases.SMALL + cases.LARGE)
def test_device_text_equals_the_model(engine, name):
    """Every pixel case through the host-pointer entry, the device entry on a window of a larger tensor (row and image pitches) and the
    tensor entry: the text is the model's, the length exact, nothing written behind it; and Pillow decodes it to exactly the pixels of
    the fixed-table text of the same input and settings."""
    import torch
    px = cases.image(name)
    h, w, _ = px.shape
    for n_, q, s in cases.GPU_CASES:
        if n_ != name:
            continue
        what = "%s q %d s %d" % (name, q, s)
        want = want_text(name, q, s)
        assert engine.jpeg_base64_bound(h, w, q, s, optimize=True) == model.base64_bound(h, w, q, s) >= len(want)
        _same(engine.encode_jpeg_base64_fit(px, q, s, optimize=True), want, what + " (host entry)")
        texts, lens = _device_entry(engine, _window(px[None]), q, s)
        assert int(lens[0]) == len(want), what
        _same(texts[0, :int(lens[0])].tobytes(), want, what + " (device entry, window)")
        assert (texts[0, int(lens[0]):] == GUARD).all(), what
        tx, ln = engine.encode_jpeg_base64_fit_tensor(torch.from_numpy(px[None]).cuda(), quality=q, sampling=s, optimize=True)
        torch.cuda.synchronize()
        _same(tx[0, :int(ln[0])].cpu().numpy().tobytes(), want, what + " (tensor entry)")
        fixed = engine.encode_jpeg_base64_fit(px, q, s, optimize=False)
        assert fixed == opt.jpeg_base64(px, q, s), what
        assert np.array_equal(_decode(want, h, w), _decode(fixed, h, w)), what


def test_three_images_in_one_call_keep_their_own_tables(engine):
    """n = 3 different images of one size (flat, noise, ramp) in one call: each text is its own image's model text, so no table leaks
    between images; lens are exact and nothing is written beyond lens[i] inside the poisoned stride."""
    h, w = 40, 56
    imgs = [np.full((h, w, 3), 180, np.uint8), cases.noise(h, w, 21), cases.ramp_noise(h, w, 3, 22)]
    for q, s in ((85, 0), (60, 2)):
        want = [model.jpeg_base64(p, q, s) for p in imgs]
        assert len(set(want)) == 3
        for order in ((0, 1, 2), (2, 0, 1)):
            texts, lens = _device_entry(engine, _window(np.stack([imgs[i] for i in order])), q, s)
            for k, i in enumerate(order):
                assert int(lens[k]) == len(want[i]), (q, s, order, k)
                _same(texts[k, :int(lens[k])].tobytes(), want[i], "image %d of %s at q %d s %d" % (k, order, q, s))
                assert (texts[k, int(lens[k]):] == GUARD).all(), (q, s, order, k)


def test_the_table_kernel_alone(engine):
    """ire_debug_jpeg_huffman on the native test's histograms (one symbol, the tie, all 162 AC symbols alike, Fibonacci counts whose
    tree is far deeper than 16, all 256 symbols) and on the real histograms of the deep case: bits and vals equal the model's."""
    hists = list(cases.synthetic_histograms().items())
    name, q, s = cases.DEEP
    hists += [("deep_%d" % t, h) for t, h in enumerate(model.image_histograms(cases.image(name), q, s))]
    hists += [("flat_%d" % t, h) for t, h in enumerate(model.image_histograms(cases.image("flat"), 85, 2))]
    while len(hists) % 4:
        hists.append(("one_more", cases.synthetic_histograms()["one"]))
    counts = np.stack([h for _, h in hists]).astype(np.uint32).reshape(-1, 4, 256)
    bv, nv = engine.debug_jpeg_huffman(counts)
    bv, nv = bv.reshape(-1, 272), nv.reshape(-1)
    assert max(model.gen_optimal_table(h)[2] for _, h in hists) > 16
    for k, (name, h) in enumerate(hists):
        bits, vals, _ = model.gen_optimal_table(h)
        assert nv[k] == len(vals) and bv[k, :16].tolist() == bits and bv[k, 16:16 + len(vals)].tolist() == vals and not bv[k, 16 + len(vals):].any(), name


@pytest.mark.parametrize("q,s", [(60, 2), (92, 2)])
def test_every_job_kind_on_an_optimising_engine(engine, q, s):
    """Engine(flags=IRE_FLAG_RESULT_JPEG | IRE_FLAG_JPEG_OPTIMIZE): a fit job, a file job, an upload job and a 2-view fusion job, all
    submitted before the first poll.  Each polled text is the model's optimised text of the PIXELS the session's pixel engine returns
    for the same submission; four distinct 48 x 64 fit jobs coalesced into one batch each get their own tables."""
    import jpeg_decode_cases as dcases
    from test_fusion_jobs_gpu import _views
    from test_submit_upload_gpu import _file
    file_job = dcases.encode(dcases.smooth(48, 64, 57), 95, 2)
    upload = _file(131, 97, "420", 6)
    views = _views(70, 90, 2)
    four = [np.full((48, 64, 3), 90, np.uint8), cases.noise(48, 64, 31), cases.ramp_noise(48, 64, 3, 32), cases.ramp_noise(48, 64, 1, 33)]
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG | _lib.IRE_FLAG_JPEG_OPTIMIZE, jpeg_quality=q, jpeg_sampling=s)
    try:
        submissions = [("fit job", lambda e: e.submit_fit(cases.image("noise"), is_jpeg=False)), ("file job", lambda e: e.submit_jpeg(file_job)),
                       ("upload job", lambda e: e.submit_upload(upload, max_dim=128)), ("fusion job", lambda e: e.submit_fuse_fit(views))]
        submissions += [("fit job %d of four of one shape" % k, (lambda p: lambda e: e.submit_fit(p, is_jpeg=False))(p)) for k, p in enumerate(four)]
        jobs = [submit(eng) for _, submit in submissions]
        got = [eng.poll(j, timeout_ms=120000) for j in jobs]
        texts = []
        for (what, submit), job, (text, scores, _) in zip(submissions, jobs, got):
            ref, ref_scores, _ = engine.poll(submit(engine), timeout_ms=120000)
            h, w = job[1], job[2]
            assert isinstance(text, bytes) and ref.shape == (h, w, 3), what
            want = model.jpeg_base64(ref, q, s)
            assert len(want) <= eng.jpeg_base64_bound(h, w) == model.base64_bound(h, w, q, s), what
            _same(text, want, what)
            assert np.array_equal(scores, ref_scores), what
            assert np.array_equal(_decode(text, h, w), _decode(opt.jpeg_base64(ref, q, s), h, w)), what
            texts.append(text)
        heads = [base64.b64decode(t)[177:400] for t in texts[4:]]
        assert len(set(heads)) == 4                       # four images, four sets of tables
    finally:
        eng.close()


_DEFAULT_SCRIPT = r"""
import hashlib, sys
import numpy as np, torch
sys.path.insert(0, %r)
from image_restoration_platform_amd import synth
from image_restoration_platform_amd.engine import Engine
eng = Engine(max_batch=8)
x = torch.from_numpy(synth.batch(8, 1024, 1024)).cuda()
def fixed():
    tx, ln = eng.encode_jpeg_base64_fit_tensor(x)
    torch.cuda.synchronize()
    tx, ln = tx.cpu().numpy(), ln.cpu().numpy()
    return hashlib.sha256(b"\n".join(tx[i, :int(ln[i])].tobytes() for i in range(8))).hexdigest(), int(ln.sum())
a = fixed()
tx, ln = eng.encode_jpeg_base64_fit_tensor(x, optimize=True)
torch.cuda.synchronize()
o = int(ln.sum().item())
b = fixed()
tx2, ln2 = eng.encode_jpeg_base64_fit_tensor(x, optimize=True)
torch.cuda.synchronize()
same = bool((ln == ln2).all().item()) and all(bool((tx[i, :int(ln[i])] == tx2[i, :int(ln2[i])]).all().item()) for i in range(8))
eng.close()
print("RESULT", a[0], b[0], a[1], o, int(same))
"""


def test_the_default_is_untouched(engine):
    """In a process of its own: the sha256 of the fixed-table texts of the bench's synthetic batch (8 x 1024 x 1024) before the optimised
    path has ever run in the process equals the one after; the optimised texts of the same batch repeat exactly (their total length is printed, not judged)."""
    r = subprocess.run([sys.executable, "-c", _DEFAULT_SCRIPT % ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    before, after, fixed_chars, opt_chars, same = next(line for line in r.stdout.splitlines() if line.startswith("RESULT")).split()[1:]
    print("fixed %s characters, optimised %s: ratio %.4f" % (fixed_chars, opt_chars, int(opt_chars) / int(fixed_chars)))
    assert before == after and int(same) == 1
    assert int(opt_chars) > 0 and int(fixed_chars) > 0
    # and in this process, where the optimised path has run: the default's text is still the fixed-table model's
    px = cases.image("noise")
    assert engine.encode_jpeg_base64_fit(px) == opt.jpeg_base64(px, 85, 0)
