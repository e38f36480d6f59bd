#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 kernels?   tools/isa_same.py OLD_TREE NEW_TREE [file.hip ...]

For every .hip in build.py's SOURCES (each tree's own build.py: COMMON plus that file's default extra flags) this compiles
device-only assembly, cuts it into kernels (body, .amdhsa_* descriptor, metadata entry) and compares the two trees as multisets
of kernel texts, per file.  Mangled names, the translation unit's __hip_cuid hash and the per-function number inside local labels
(.LBB3_7, and BB3_7 in the loop comments) are replaced by placeholders first, so a renamed kernel or a shorter template argument list is no difference; anything else is.
Exit status 1 if a kernel exists only in the new tree (kernels only in the old tree are listed: instantiations that were removed).
"""
import collections
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

PKG = "image_restoration_platform_amd"
BEGIN = re.compile(r"; -- Begin function (\S+)")
NORMALISE = [(re.compile(r"_Z[A-Za-z0-9_]+"), "_ZNAME"), (re.compile(r"__hip_cuid_[0-9a-f]+"), "__hip_cuid_HASH"),
             (re.compile(r"(\.L[A-Za-z_]+?)\d+(_\d+)?\b"), r"\1\2"), (re.compile(r"\bBB\d+_(\d+)"), r"BB_\1")]


def load_build(tree):
    spec = importlib.util.spec_from_file_location("ire_build_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, src, extra, tmp):
    out = os.path.join(tmp, src + ".s")
    cmd = [build._hipcc()] + build.COMMON + extra + ["-x", "hip", "--cuda-device-only", "-S", os.path.join(build.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed for %s:\n%s" % (os.path.join(build.CSRC, src), r.stderr[-3000:]))
    return open(out).read()


def kernels(text):
    """{mangled name: [normalised text, ...]}: function body with its descriptor, plus its entry in amdhsa.kernels."""
    code, _, meta = text.partition("\t.amdgpu_metadata")
    code = code.split("\t.section\t.AMDGPU.gpr_maximums")[0]
    parts = collections.defaultdict(list)
    name = None
    for line in code.splitlines():
        m = BEGIN.search(line)
        name = m.group(1) if m else name
        if name and not line.startswith("\t.section\t.text"):      # the section line holds nothing but the name
            parts[name].append(line)
    entries = re.split(r"^  - ", meta.split("amdhsa.target:")[0], flags=re.M)[1:]
    for e in entries:
        parts[re.search(r"\.name:\s+(\S+)", e).group(1)].append(e)
    out = {}
    for name, lines in parts.items():
        t = "\n".join(lines)
        for rx, to in NORMALISE:
            t = rx.sub(to, t)
        out[name] = t
    return out


def demangle(names):
    if not names:
        return []
    try:
        return subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return names


def main(old_tree, new_tree, only):
    old_b, new_b = load_build(os.path.abspath(old_tree)), load_build(os.path.abspath(new_tree))
    old_flags = dict(old_b.SOURCES)
    files = [(s, f) for s, f in new_b.SOURCES if s.endswith(".hip") and (not only or s in only)]
    jobs = {}
    with tempfile.TemporaryDirectory() as t_old, tempfile.TemporaryDirectory() as t_new, \
            concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for s, f in files:
            jobs[s] = (ex.submit(assembly, old_b, s, old_flags.get(s, []), t_old), ex.submit(assembly, new_b, s, f, t_new))
        added = 0
        for s, _ in files:
            old, new = kernels(jobs[s][0].result()), kernels(jobs[s][1].result())
            left = collections.defaultdict(list)             # normalised text -> names in the old tree not yet matched
            for n, t in old.items():
                left[t].append(n)
            only_new = [n for n, t in new.items() if not (left[t] and left[t].pop())]
            only_old = [n for ns in left.values() for n in ns]
            print("%-18s %3d identical, %d only in old, %d only in new" % (s, len(new) - len(only_new), len(only_old), len(only_new)))
            for tag, names in (("old", only_old), ("new", only_new)):
                for d in sorted(demangle(names)):
                    print("    only in %s: %s" % (tag, d))
            added += len(only_new)
    return 1 if added else 0


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
