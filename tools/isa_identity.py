#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 machine code? (CPU only: needs hipcc, no GPU.)

usage: python tools/isa_identity.py <tree A> <tree B> [--nb N] [--out DIR] [--allow-new] [--ignore-kernarg-size]

Builds the device assembly of both trees (csrc/build.sh --cuda-device-only -S; --nb N adds -DSMPC_ONLY_NB=N: seconds
instead of a minute), splits it into functions and `.amdhsa_kernel` descriptors (register counts, LDS, scratch and
kernarg sizes) and compares them name by name, whatever their order in the file. Exit status 1 on any difference or
unpaired function; the normalised texts of a differing pair are left under --out for diff(1).

--allow-new: a function or descriptor that only tree B has is listed as NEW and is no failure (B adds kernels, and A's
must come out unchanged). --ignore-kernarg-size: `.amdhsa_kernarg_size` lines are left out of the descriptor comparison and
the kernels whose size changed are counted (members appended to KParams, which every sweep kernel takes by value, grow the
kernel-argument segment of all of them without moving an existing member)."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

BUILD = os.path.join("nav2_social_mpc_controller_amd", "csrc", "build.sh")

# Names of tree A that tree B spells differently, applied to A's text before anything is compared (so a name inside a
# body is compared under its new spelling too). Written out, not inferred from matching bodies.
_TAIL = r"EEvNS_7KParamsE"
RENAMES = [
    # smpc_solve_sp_kernel<NB,W> -> smpc_solve_kernel<NB,W,true,true>; smpc_solve_kernel<NB,W,vt> -> <NB,W,vt,false>
    (r"_ZN4smpc20smpc_solve_sp_kernelILi(\d+)ELi(\d+)E" + _TAIL, r"_ZN4smpc17smpc_solve_kernelILi\1ELi\2ELb1ELb1E" + _TAIL),
    (r"_ZN4smpc17smpc_solve_kernelILi(\d+)ELi(\d+)ELb([01])E" + _TAIL, r"_ZN4smpc17smpc_solve_kernelILi\1ELi\2ELb\3ELb0E" + _TAIL),
    # smpc_eval_sp_kernel<NB,W> -> smpc_eval_kernel<NB,W,true,true>; smpc_eval_kernel<NB,W,vt> -> <NB,W,vt,false>
    (r"_ZN4smpc19smpc_eval_sp_kernelILi(\d+)ELi(\d+)E" + _TAIL, r"_ZN4smpc16smpc_eval_kernelILi\1ELi\2ELb1ELb1E" + _TAIL),
    (r"_ZN4smpc16smpc_eval_kernelILi(\d+)ELi(\d+)ELb([01])E" + _TAIL, r"_ZN4smpc16smpc_eval_kernelILi\1ELi\2ELb\3ELb0E" + _TAIL),
    # smpc_solve_kernel<NB,W,vt,sp> -> <NB,W,vt,sp,false>; smpc_solve_trace_kernel<NB,W> -> smpc_solve_kernel<NB,W,true,true,true>
    (r"_ZN4smpc17smpc_solve_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])E" + _TAIL, r"_ZN4smpc17smpc_solve_kernelILi\1ELi\2ELb\3ELb\4ELb0E" + _TAIL),
    (r"_ZN4smpc23smpc_solve_trace_kernelILi(\d+)ELi(\d+)E" + _TAIL, r"_ZN4smpc17smpc_solve_kernelILi\1ELi\2ELb1ELb1ELb1E" + _TAIL),
    # smpc_crowd_step_kernel -> smpc_crowd_step_kernel<false, CrowdParams> (kGroups = true is the groups kernel)
    (r"_ZN4smpc22smpc_crowd_step_kernelENS_11CrowdParamsE", r"_ZN4smpc22smpc_crowd_step_kernelILb0ENS_11CrowdParamsEEEvT0_"),
    # (smpc_solve_fixed_kernel<FixedShape<T, N, CH, bl>> and smpc_eval_fixed_kernel<...> stand beside smpc_solve_kernel /
    # smpc_eval_kernel, whose names did not change: against a tree without them they are NEW under --allow-new)
]
# what cannot matter: the numbers the compiler gives basic blocks, temporaries, jump tables and function ends
LABELS = [(r"\.LBB\d+_", ".LBB_"), (r"\.Ltmp\d+", ".Ltmp"), (r"\.LJTI\d+_", ".LJTI_"), (r"\.LCPI\d+_", ".LCPI_"),
          (r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1")]


def start_build(tree, nb, out):
    cmd = ["bash", os.path.join(tree, BUILD), "--cuda-device-only", "-S"] + ([f"-DSMPC_ONLY_NB={nb}"] if nb else [])
    return subprocess.Popen(cmd, env={**os.environ, "SMPC_OUT": out})


def split(text):
    """({symbol: normalised body lines}, {kernel symbol: descriptor lines}) of one assembly file."""
    funcs, descs, name, desc, is_function = {}, {}, None, None, set()
    for raw in text.splitlines():
        line = raw.split(";")[0].rstrip()  # comments name basic blocks by their numbers
        if not line:
            continue
        if re.match(r"\s*\.(text|section)\b", line):  # a template's code goes to a section of its own (comdat): not code
            continue
        for pat, rep in LABELS:
            line = re.sub(pat, rep, line)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            desc = descs.setdefault(m.group(1), [])
        if desc is not None:  # a descriptor may sit inside its function's text: it is compared on its own
            desc.append(line.strip())
            if line.strip() == ".end_amdhsa_kernel":
                desc = None
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            is_function.add(m.group(1))
        m = re.match(r"([^\s:]+):", line)
        if m and name is None and m.group(1) in is_function:  # (data labels and the metadata's keys are not code)
            name = m.group(1)
            funcs[name] = []
        if name is not None:
            funcs[name].append(line)
            if line.startswith(".Lfunc_end"):
                name = None
    return funcs, descs


def n_instructions(lines):
    return sum(1 for l in lines if l[:1] in " \t" and not l.strip().startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a"), ap.add_argument("tree_b"), ap.add_argument("--nb", type=int)
    ap.add_argument("--out", default=None, help="directory for the texts of differing functions")
    ap.add_argument("--allow-new", action="store_true", help="names only tree B has are no failure")
    ap.add_argument("--ignore-kernarg-size", action="store_true", help="compare descriptors without .amdhsa_kernarg_size")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        files = [os.path.join(tmp, "a.s"), os.path.join(tmp, "b.s")]
        jobs = [start_build(t, args.nb, f) for t, f in zip((args.tree_a, args.tree_b), files)]  # two compiler jobs
        if any(j.wait() != 0 for j in jobs):
            sys.exit("build failed")
        text_a, text_b = (open(f).read() for f in files)
    for pat, rep in RENAMES:
        text_a = re.sub(pat, rep, text_a)
    (fa, da), (fb, db) = split(text_a), split(text_b)
    bad = new = resized = 0
    if args.ignore_kernarg_size:
        size = lambda d: [l for l in d if l.startswith(".amdhsa_kernarg_size")]
        resized = sum(1 for n in set(da) & set(db) if size(da[n]) != size(db[n]))
        da, db = ({n: [l for l in d if not l.startswith(".amdhsa_kernarg_size")] for n, d in x.items()} for x in (da, db))
    for kind, a, b in (("function", fa, fb), ("descriptor", da, db)):
        for name in sorted(set(a) | set(b)):
            if args.allow_new and name not in a:
                verdict = "NEW (only in B)"
                new += 1
            elif name not in a or name not in b:
                verdict = "UNPAIRED (only in %s)" % ("A" if name in a else "B")
            else:
                verdict = "same" if a[name] == b[name] else "DIFFERENT"
            lines = a.get(name) or b.get(name)
            print(f"{kind} {name} {n_instructions(lines) if kind == 'function' else len(lines)} {verdict}")
            if verdict not in ("same", "NEW (only in B)"):
                bad += 1
                out = args.out or tempfile.mkdtemp(prefix="isa_identity_")
                args.out = out
                os.makedirs(out, exist_ok=True)
                for side, d in (("a", a), ("b", b)):
                    with open(os.path.join(out, f"{kind}.{name[:150]}.{side}.s"), "w") as f:
                        f.write("\n".join(d.get(name, [])) + "\n")
    print(f"{len(set(fa) | set(fb))} functions, {len(set(da) | set(db))} kernel descriptors: "
          + ("all same" if not bad else f"{bad} DIFFERENT or unpaired, texts in {args.out}")
          + (f"; {new} only in B" if new else "") + (f"; .amdhsa_kernarg_size (not compared) differs in {resized} descriptors" if resized else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
