#!/usr/bin/env python3
"""Device assembly of the working tree against another revision's, kernel by kernel (CPU only, no GPU needed).
Usage: python tools/isa_diff.py PARENT_REV [--src bvh_trace.hip,kd_trace.hip,interaction.hip]

PARENT_REV's nn_bvh_amd/csrc and include are unpacked into a temporary directory (git archive); each source is
compiled there and in the tree with the product's code generation flags, and per kernel the report says `same` or
shows the first differing line; the rest of the file (metadata) is covered by a comparison of the whole file.  Lines
that carry the compilation unit's hash (__hip_cuid_) are left out, and so is the number the compiler gives a function
by its place in the file (.LBB28_3, BB28_5, .Lfunc_end28): a kernel that leaves or joins a file renumbers those behind it.
--kernarg: differences that come from a changed kernel-argument struct (offset of a scalar load from the kernarg
segment, kernarg size, .offset / .size of the argument metadata) count as `same`; they are counted and reported.
The register, spill, scratch and LDS figures of the metadata are compared in either mode.  Exit status 1 if a
kernel differs or the sets of kernels differ."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("nn_bvh_amd", "csrc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-S", "--cuda-device-only"]
FIGURES = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
           "group_segment_fixed_size")
# what may differ under --kernarg, with the part that differs blanked
KERNARG = [(re.compile(r"^(\s*s_load_dword\w*\s+\S+,\s*s\[\d+:\d+\],\s*)0x[0-9a-f]+"), r"\1OFF"),
           (re.compile(r"^(\s*\.amdhsa_kernarg_size)\s+\d+"), r"\1 N"),
           (re.compile(r"^(\s*\.kernarg_segment_size:)\s+\d+"), r"\1 N"),
           (re.compile(r"^(\s*-?\s*\.(offset|size):)\s+\d+"), r"\1 N")]
FUNC_NUMBER = re.compile(r"((?:\.L|\b)BB|\.Lfunc_begin|\.Lfunc_end)\d+")


def assemble(root, src, out):
    subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-o", out, os.path.join(root, CSRC, src)], check=True,
                   stderr=subprocess.DEVNULL)
    # (a label's comment is padded to a column, so a number that loses a digit moves it: one space there)
    return [re.sub(r"\s+;", " ;", FUNC_NUMBER.sub(r"\1N", ln)) for ln in open(out).read().splitlines()
            if "__hip_cuid_" not in ln]


def kernels(lines):
    """name -> the kernel's lines, label to .Lfunc_end (the code and, before the end label, its .amdhsa_kernel block)"""
    out = {}
    for name in [m.group(1) for ln in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]:
        start = next(k for k, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(k for k in range(start, len(lines)) if lines[k].startswith(".Lfunc_end"))
        out[name] = lines[start:end + 1]
    return out


def figures(lines):
    """name -> the FIGURES of the kernel's entry in amdhsa.kernels"""
    text = "\n".join(lines)
    out = {}
    for block in text[text.index("amdhsa.kernels:"):].split("  - .agpr_count:")[1:]:
        get = lambda k: re.search(rf"\.{k}:\s*(\S+)", block).group(1)  # noqa: E731
        out[get("name")] = tuple(get(k) for k in FIGURES)
    return out


def compare(a, b, kernarg):
    """first differing line (or None) and the number of lines that differ only in kernel-argument layout"""
    if len(a) != len(b):
        return f"{len(a)} lines against {len(b)}", 0
    moved = 0
    for x, y in zip(a, b):
        if x == y:
            continue
        if kernarg and any(rx.sub(to, x) == rx.sub(to, y) and rx.match(x) for rx, to in KERNARG):
            moved += 1
            continue
        return f"- {x.strip()}\n      + {y.strip()}", moved
    return None, moved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev")
    ap.add_argument("--src", default="bvh_trace.hip,kd_trace.hip,interaction.hip")
    ap.add_argument("--kernarg", action="store_true")
    ap.add_argument("--quiet", action="store_true", help="one line per source unless a kernel differs")
    args = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as td:
        tar = subprocess.run(["git", "-C", ROOT, "archive", args.rev, CSRC, "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", td], input=tar.stdout, check=True)
        for src in args.src.split(","):
            old = assemble(td, src, os.path.join(td, "old.s"))
            new = assemble(ROOT, src, os.path.join(td, "new.s"))
            ko, kn, fo, fn = kernels(old), kernels(new), figures(old), figures(new)
            for name in sorted(set(ko) ^ set(kn)):
                print(f"{src}: {name}: only in {'the tree' if name in kn else args.rev}")
                bad += 1
            moved_all = 0
            for name in sorted(set(ko) & set(kn)):
                diff, moved = compare(ko[name], kn[name], args.kernarg)
                if fo[name] != fn[name]:
                    diff = f"{FIGURES}: {fo[name]} against {fn[name]}"
                moved_all += moved
                if diff or not args.quiet:
                    print(f"{src}: {name}: {'same' if not diff else 'DIFFERS'}" + (f" ({moved} kernarg lines)" if moved else ""))
                if diff:
                    print("      " + diff)
                    bad += 1
            whole, moved = compare(old, new, args.kernarg)
            print(f"{src}: {len(kn)} kernels, {len(old)} / {len(new)} lines, {moved} differ in kernel-argument layout "
                  f"({moved_all} of them inside kernels); {'no other difference' if not whole else 'DIFFERS: ' + whole}")
            bad += 1 if whole else 0
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
