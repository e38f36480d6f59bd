"""How an engine's flags come about for ICC-tagged uploads (engine.upload_icc_flags, what Engine.__init__ passes to ire_init):
upload_icc=True adds IRE_FLAG_UPLOAD_ICC; IRE_UPLOAD_ICC=1 in the environment adds it for every engine that does not say
upload_icc=False; no other value of the variable does; the other flags pass through.  No engine, no GPU."""
from image_restoration_platform_amd import _lib
from image_restoration_platform_amd.engine import upload_icc_flags

ICC = _lib.IRE_FLAG_UPLOAD_ICC
PROG = _lib.IRE_FLAG_DECODE_PROGRESSIVE


def test_upload_icc_flag_from_argument_and_environment():
    assert ICC == 256 and ICC & (ICC - 1) == 0
    assert upload_icc_flags(0, None, {}) == 0
    assert upload_icc_flags(PROG, None, {}) == PROG
    assert upload_icc_flags(PROG, True, {}) == PROG | ICC
    assert upload_icc_flags(PROG, None, {"IRE_UPLOAD_ICC": "1"}) == PROG | ICC
    assert upload_icc_flags(PROG, False, {"IRE_UPLOAD_ICC": "1"}) == PROG
    for other in ("0", "", "true", "yes", "2"):
        assert upload_icc_flags(0, None, {"IRE_UPLOAD_ICC": other}) == 0
    assert upload_icc_flags(ICC, False, {}) == ICC              # a flag given as a flag is never taken away
    assert upload_icc_flags(ICC | PROG, None, {}) == ICC | PROG


def test_upload_icc_flag_reads_the_process_environment(monkeypatch):
    monkeypatch.setenv("IRE_UPLOAD_ICC", "1")
    assert upload_icc_flags(0) == ICC
    monkeypatch.delenv("IRE_UPLOAD_ICC")
    assert upload_icc_flags(0) == 0
