#!/usr/bin/env python3
"""Machine-code identity of two source trees' kura_kernels.hip.

    python tools/code_object_identity.py PARENT_TREE NEW_TREE [--work DIR] [--jobs J]

Builds both trees' dbs-gym_amd/csrc/kura_kernels.hip with build()'s hipcc and
HIP_FLAGS in four variants (plain, -DKURA_DEBUG, -DKURA_STAMPS,
-DKURA_STAMPS -DKURA_STAMPS_SI), extracts the gfx950 code object of each
(check_store_hazards.code_object) and compares the SHA-256 of the sections
that hold code and data the GPU runs: .text, .rodata, .note, .data.rel.ro.
Whole files are not compared: two builds of the same source differ in
.dynsym / .dynstr / .strtab / .hash / .gnu.hash (a per-compile id in a symbol
name).  Where .text differs, the per-symbol digests that differ are listed
to localise it.  Prints the report (profiles/r08_refactor_identity.txt is
one); exit status 1 if any section differs.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from __graft_entry__ import HIP_FLAGS, HIPCC  # noqa: E402
from check_store_hazards import LLVM, code_object  # noqa: E402

VARIANTS = (("plain", []), ("debug", ["-DKURA_DEBUG"]), ("stamps", ["-DKURA_STAMPS"]),
            ("stamps_si", ["-DKURA_STAMPS", "-DKURA_STAMPS_SI"]))
SECTIONS = (".text", ".rodata", ".note", ".data.rel.ro")


def build(tree: str, out: str, extra: list[str], reuse: bool = False) -> str:
    if reuse and os.path.exists(out):
        return out
    subprocess.run([HIPCC, *HIP_FLAGS, *extra, "-o", out, os.path.join(tree, "dbs-gym_amd", "csrc", "kura_kernels.hip")],
                   check=True)
    return out


def sections(co: str, work: str) -> dict[str, bytes]:
    out = {}
    for s in SECTIONS:
        f = os.path.join(work, os.path.basename(co) + s.replace(".", "_"))
        if os.path.exists(f):
            os.remove(f)
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section={s}={f}", co, os.path.join(work, "_discard.o")],
                       check=True, capture_output=True)
        with open(f, "rb") as fh:
            out[s] = fh.read()
    return out


def text_symbols(co: str, text: bytes) -> dict[str, str]:
    """SHA-256 of every function's bytes in .text (symbol names without the per-compile id suffix kept as is)."""
    hdr = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-W", co], check=True, capture_output=True, text=True).stdout
    base = next(int(ln.split("]")[1].split()[2], 16) for ln in hdr.splitlines() if " .text " in ln)
    syms = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for ln in syms.splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            a, n = int(f[1], 16) - base, int(f[2], 0)
            out[f[7]] = hashlib.sha256(text[a:a + n]).hexdigest()
    return out


def main(argv) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--work", default=None, help="directory for the libraries (kept); default: a temporary one")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--reuse-parent", action="store_true", help="keep the parent libraries already in --work")
    ap.add_argument("--variants", default=",".join(v for v, _ in VARIANTS), help="comma-separated subset (a quick look)")
    a = ap.parse_args(argv)
    variants = [(v, extra) for v, extra in VARIANTS if v in a.variants.split(",")]
    tmp = None if a.work else tempfile.TemporaryDirectory()
    work = a.work or tmp.name
    os.makedirs(work, exist_ok=True)
    ver = subprocess.run([HIPCC, "--version"], check=True, capture_output=True, text=True).stdout
    print("\n".join(ln for ln in ver.splitlines() if "version" in ln))
    print("flags:", " ".join(HIP_FLAGS))
    jobs = [(side, tree, v, extra) for side, tree in (("parent", a.parent), ("new", a.new)) for v, extra in variants]
    with ThreadPoolExecutor(a.jobs) as ex:
        libs = list(ex.map(lambda j: build(j[1], os.path.join(work, f"{j[0]}_{j[2]}.so"), j[3],
                                           a.reuse_parent and j[0] == "parent"), jobs))
    secs = {(j[0], j[2]): sections(code_object(lib, work), work) for j, lib in zip(jobs, libs)}
    bad = 0
    for v, extra in variants:
        print(f"\n== {v} ({' '.join(extra) or 'no extra flags'})")
        for s in SECTIONS:
            p, n = secs[("parent", v)][s], secs[("new", v)][s]
            same = p == n
            bad += not same
            print(f"{s:13s} parent {len(p):8d} B {hashlib.sha256(p).hexdigest()}")
            print(f"{'':13s} new    {len(n):8d} B {hashlib.sha256(n).hexdigest()}  {'identical' if same else 'DIFFERENT'}")
        if secs[("parent", v)][".text"] != secs[("new", v)][".text"]:
            ps = text_symbols(os.path.join(work, f"parent_{v}.so.gfx950.o"), secs[("parent", v)][".text"])
            ns = text_symbols(os.path.join(work, f"new_{v}.so.gfx950.o"), secs[("new", v)][".text"])
            for k in sorted(set(ps) | set(ns)):
                if ps.get(k) != ns.get(k):
                    print(f"  differs: {k}")
    print("\nresult:", "all sections identical in all variants" if not bad else f"{bad} section(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
