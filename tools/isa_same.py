#!/usr/bin/env python3
"""Is the device code of a translation unit the same in two source trees?  The check of a refactor, without a GPU.

usage: isa_same.py OLD_TREE NEW_TREE file.hip ...
Compiles magcache_amd/csrc/<file> of both trees to gfx950 assembly with the project's own flags (NEW_TREE's build.FLAGS +
EXTRA_FLAGS for that file; a file of the reference library is also compiled with -DMC_WITH_REF_GEMM), reduces both to
instruction lines (comments and directives stripped, block labels renumbered per kernel) and compares, per kernel matched
by demangled name: the instruction sequence, .amdhsa_next_free_vgpr / _sgpr, .amdhsa_group_segment_fixed_size and
.amdhsa_private_segment_fixed_size.  Kernels whose name exists in one tree only are paired in order of appearance and the
pairing is printed.  It only diffs.  Exit status 1 if anything differs."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

KEYS = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size",
        ".amdhsa_private_segment_fixed_size")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("mc_build", os.path.join(tree, "magcache_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assembly(build, tree, src, extra, tmp):
    out = os.path.join(tmp, "out.s")
    subprocess.check_call([build.HIPCC] + build.FLAGS + extra + build.EXTRA_FLAGS.get(src, []) +
                          ["--cuda-device-only", "-S", os.path.join(tree, "magcache_amd", "csrc", src), "-o", out])
    return open(out).read().splitlines()


def kernels(lines, cxxfilt):
    """{demangled name: (instruction lines, {directive: value})}, in order of appearance"""
    meta, cur = {}, None
    for l in lines:
        t = l.strip()
        if t.startswith(".amdhsa_kernel "):
            cur = meta.setdefault(t.split()[1], {})
        elif t == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and t.split()[0] in KEYS:
            cur[t.split()[0]] = t.split()[1]
    found, body = [], None
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$]*):", l)
        if m and m.group(1) in meta:
            body, labels = [], {}
            found.append((m.group(1), body))
            continue
        if body is None:
            continue
        t = l.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = ".L%d" % len(labels)
            body.append(m.group(1) + ":")
        elif t.startswith(".Lfunc_end"):   # forward branches are known now: renumber the labels
            body[:] = [re.sub(r"\.LBB\d+_\d+", lambda k: labels.get(k.group(0), k.group(0)), x) for x in body]
            body = None
        elif t and not t.startswith("."):
            body.append(t)
    names = subprocess.run([cxxfilt], input="\n".join(n for n, _ in found), capture_output=True, text=True,
                           check=True).stdout.splitlines()
    return {d: (b, meta[n]) for d, (n, b) in zip(names, found)}


def main():
    old_tree, new_tree, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    build = load_build(new_tree)
    cxxfilt = os.environ.get("CXXFILT", "c++filt")
    bad = 0
    for src in files:
        variants = ([[]] if src in build.SOURCES else []) + \
                   ([["-DMC_WITH_REF_GEMM"]] if src in build.REF_RECOMPILED + build.REF_EXTRA else [])
        for extra in variants or [[]]:
            with tempfile.TemporaryDirectory() as tmp:
                old = kernels(assembly(build, old_tree, src, extra, tmp), cxxfilt)
                new = kernels(assembly(build, new_tree, src, extra, tmp), cxxfilt)
            pairs = [(k, k) for k in old if k in new]
            only_old, only_new = [k for k in old if k not in new], [k for k in new if k not in old]
            for a, b in zip(only_old, only_new):
                print(f"  paired by position: {a}  ->  {b}")
                pairs.append((a, b))
            unpaired = only_old[len(only_new):] + only_new[len(only_old):]
            diff = []
            for a, b in pairs:
                (oi, om), (ni, nm) = old[a], new[b]
                if oi != ni:
                    at = next((i for i, (x, y) in enumerate(zip(oi, ni)) if x != y), min(len(oi), len(ni)))
                    diff.append(f"{a}: {len(oi)} -> {len(ni)} instruction lines, first difference at {at}: "
                                f"'{oi[at] if at < len(oi) else ''}' | '{ni[at] if at < len(ni) else ''}'")
                if om != nm:
                    diff.append(f"{a}: resources {om} -> {nm}")
            n_ins = sum(len(new[b][0]) for _, b in pairs)
            tag = src + (" " + " ".join(extra) if extra else "")
            if diff or unpaired:
                bad += 1
                print(f"DIFFERENT {tag}:\n  " + "\n  ".join(diff + [f"unpaired: {u}" for u in unpaired]))
            else:
                print(f"same      {tag}: {len(pairs)} kernels, {n_ins} instruction lines, resources equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
