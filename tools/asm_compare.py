#!/usr/bin/env python3
"""Per-kernel device-assembly comparison of two trees: tools/asm_compare.py TREE_A TREE_B SRC [SRC ...] [--probes]

Each SRC (csrc/SRC.hip, where a tree has it) is compiled to gfx950 assembly with exactly the flags that tree's
tfhe-gpu_amd/Makefile gives its object (`make -n`), or with --probes its test-library object build/SRC_probes.o
(a source without one falls back to its product object, which is what the test library links).  The kernels of
all the sources are pooled per tree and compared by name, so a kernel may move between files.  Only text is
compared: labels are renumbered, comments and debug-location lines dropped; a kernel's .amdhsa descriptor
(registers, scratch, LDS) is part of its text.  Prints the kernels that differ and exits 1 if any does.
"""
import argparse, difflib, os, re, shlex, shutil, subprocess, sys, tempfile


def compile_cmd(tree, src, probes):
    d = os.path.join(tree, "tfhe-gpu_amd")
    for obj in ([f"build/{src}_probes.o"] if probes else []) + [f"build/{src}.o"]:
        r = subprocess.run(["make", "-n", "-B", obj], cwd=d, capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if " -c " in l and f"csrc/{src}." in l]
        if r.returncode == 0 and lines:
            return d, shlex.split(lines[0])
    sys.exit(f"{tree}: no rule builds {src}")


def assembly(tree, src, probes, keep, reuse):
    d, cmd = compile_cmd(tree, src, probes)
    out = os.path.join(keep, f"{os.path.basename(os.path.abspath(tree))}_{src}{'_probes' if probes else ''}.s")
    if not (reuse and os.path.exists(out)):
        cmd[cmd.index("-o") + 1] = out
        cmd[cmd.index("-c")] = "-S"
        subprocess.run(cmd + ["--cuda-device-only"], cwd=d, check=True)
    return open(out).read()


def kernels(text):
    """name -> normalised lines of every kernel (body + descriptor)"""
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names and cur is None:
            cur = out.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        if cur is None:
            continue
        s = line.split(";")[0].rstrip()
        if s and not re.match(r"^\s*\.(loc|file|cfi_\w+|p2align)\b", s):
            cur.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?", lambda k: ".L" + k.group(1) + (k.group(2) or ""), s))
        if re.match(r"^\.Lfunc_end\d+:", line) or ".end_amdhsa_kernel" in line:
            cur = None
    return out


def demangle(names):
    try:
        r = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"] + names, capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("tree_a"), ap.add_argument("tree_b"), ap.add_argument("src", nargs="+")
    ap.add_argument("--probes", action="store_true", help="the test library's objects (-DTFHE_TEST_PROBES)")
    ap.add_argument("--keep", help="directory for the .s files (default: a temporary one)")
    ap.add_argument("--reuse-a", action="store_true", help="with --keep: do not recompile TREE_A's .s files found there")
    ap.add_argument("--diff",action="store_true", help="print a unified diff of each differing kernel")
    a = ap.parse_args()
    keep = os.path.abspath(a.keep) if a.keep else tempfile.mkdtemp(prefix="asm_compare_")
    os.makedirs(keep, exist_ok=True)
    pools = []
    for tree in (a.tree_a, a.tree_b):
        pool = {}
        for src in a.src:
            if os.path.exists(os.path.join(tree, "tfhe-gpu_amd", "csrc", src + ".hip")):
                pool.update(kernels(assembly(tree, src, a.probes, keep, a.reuse_a and tree == a.tree_a)))
        pools.append(pool)
    A, B = pools
    pretty = demangle(sorted(set(A) | set(B)))
    bad = 0
    for n in sorted(set(A) | set(B)):
        if n not in A or n not in B:
            print(f"ONLY IN {'A' if n in A else 'B'}: {pretty[n]}")
            bad += 1
        elif A[n] != B[n]:
            d = list(difflib.unified_diff(A[n], B[n], "A", "B", lineterm="", n=1))
            changed = sum(1 for l in d if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print(f"DIFFERS ({changed} lines): {pretty[n]}")
            if a.diff:
                print("\n".join(d))
            bad += 1
    print(f"{len(set(A) & set(B))} kernels in both trees ({'test' if a.probes else 'product'} build), {bad} differ or are missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
