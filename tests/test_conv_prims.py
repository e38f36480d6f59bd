"""The wave-level primitives of the convolution kernels live once, in csrc/conv_prims.hpp (DESIGN.md "kernels"): a kernel file
includes them and defines none of its own.  Source text only -- what keeps the next forked kernel from bringing the copies back."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image_restoration_platform_amd", "csrc")
KERNELS = sorted(glob.glob(os.path.join(CSRC, "conv_*.hip")))
# the LDS-DMA load and the two permlane swaps: wait states and M0 handling by hand, explained where they are defined
DELICATE = ("global_load_lds_dwordx4", "v_permlane16_swap_b32", "v_permlane32_swap_b32")
HOMES = {"conv_prims.hpp", "gn_fold.hpp"}          # gn_fold.hpp: the double-precision cross-lane add, a function of its own
COPY = re.compile(r"__device__[^;{}()]*?\b(\w+_(?:pack|glds16|ror_add|swap16_add|swap32_add))\s*\(")


def _text(path):
    with open(path) as f:
        return f.read()


def test_every_conv_kernel_includes_the_primitives():
    assert len(KERNELS) >= 11
    missing = [os.path.basename(p) for p in KERNELS if '#include "conv_prims.hpp"' not in _text(p)]
    assert not missing, missing


def test_delicate_asm_lives_in_one_place():
    found = {}
    for path in glob.glob(os.path.join(CSRC, "*")):
        text = _text(path) if os.path.isfile(path) else ""
        for s in DELICATE:
            if s in text:
                found.setdefault(s, set()).add(os.path.basename(path))
    assert set(found) == set(DELICATE) and all("conv_prims.hpp" in f for f in found.values()), found
    strays = {s: sorted(f - HOMES) for s, f in found.items() if f - HOMES}
    assert not strays, strays


def test_no_kernel_defines_a_prefixed_copy():
    copies = {os.path.basename(p): COPY.findall(_text(p)) for p in KERNELS}
    copies = {k: v for k, v in copies.items() if v}
    assert not copies, copies
