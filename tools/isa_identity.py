#!/usr/bin/env python3
"""Check that a change leaves every pre-existing kernel machine-identical: compile mlkem_capi.hip of a base revision and of the
working tree with build.py's HIPCC_FLAGS plus --save-temps and -Rpass-analysis=kernel-resource-usage (no GPU needed), then compare,
for every kernel symbol of the base, the instruction text between its label and its .Lfunc_end label, and its resource-usage
remarks.  Kernels that exist only in the working tree are listed, not compared.

    python tools/isa_identity.py --base HEAD~1                      # compiles both (a few minutes each)
    python tools/isa_identity.py --base-s A.s --base-remarks A.txt --new-s B.s --new-remarks B.txt
Exit status 0 when every base kernel is identical."""
import argparse
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "crystals-kyber_amd"))


def compile_tree(src_root, out_dir):
    import build
    cmd = [build.hipcc_path(), *build.HIPCC_FLAGS, "-fPIC", "-shared", "--save-temps", "-Rpass-analysis=kernel-resource-usage",
           "-o", os.path.join(out_dir, "lib.so"), os.path.join(src_root, "crystals-kyber_amd", "csrc", "mlkem_capi.hip")]
    r = subprocess.run(cmd, cwd=out_dir, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("compile failed in %s:\n%s" % (src_root, r.stderr[-4000:]))
    s = glob.glob(os.path.join(out_dir, "*gfx950*.s"))
    assert len(s) == 1, s
    return s[0], r.stderr


def kernels(asm):
    """symbol -> instruction text from its label to .Lfunc_end (comments and blank lines dropped, local label numbers dropped)"""
    out, cur, body = {}, None, []
    for line in asm.splitlines():
        if cur is None:
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[cur] = "\n".join(body)
            cur = None
            continue
        t = line.split(";")[0].rstrip()
        if t:   # local labels are numbered by the function's position in the file: compare them without the number
            body.append(re.sub(r"\.(LBB|Ltmp|Lfunc_end)\d+", r".\1", t))
    return out


def remarks(text):
    """symbol -> its resource-usage remark lines (file positions dropped)"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur and "remark:" in line:   # "<file>:<line>:<col>: <item>" -> "<item>"
            out[cur].append(re.sub(r"^.*?:\d+:\d+:\s*", "", line.split("remark:", 1)[1]).strip())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", help="git revision to compare against (e.g. HEAD~1, the parent of the change)")
    ap.add_argument("--base-s"), ap.add_argument("--base-remarks"), ap.add_argument("--new-s"), ap.add_argument("--new-remarks")
    a = ap.parse_args()
    if not a.base and not a.base_s:
        ap.error("give --base REV (the revision before the change), or the four prebuilt files")
    if a.base_s:
        bs, br = open(a.base_s).read(), open(a.base_remarks).read()
        ns, nr = open(a.new_s).read(), open(a.new_remarks).read()
    else:
        with tempfile.TemporaryDirectory() as t:
            base_root = os.path.join(t, "base")
            os.makedirs(base_root)
            arch = subprocess.run(["git", "-C", ROOT, "archive", a.base, "crystals-kyber_amd", "include"], capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", base_root], input=arch.stdout, check=True)
            for name, root in (("base", base_root), ("new", ROOT)):
                d = os.path.join(t, "out_" + name)
                os.makedirs(d)
                s_path, rem = compile_tree(root, d)
                if name == "base":
                    bs, br = open(s_path).read(), rem
                else:
                    ns, nr = open(s_path).read(), rem
    kb, kn, rb, rn = kernels(bs), kernels(ns), remarks(br), remarks(nr)
    differ = [k for k in kb if kn.get(k) != kb[k]]
    rdiffer = [k for k in kb if rn.get(k) != rb.get(k)]
    added = sorted(k for k in kn if k not in kb)
    print("base kernels: %d, identical instruction text: %d, identical resource usage: %d" %
          (len(kb), len(kb) - len(differ), len(kb) - len(rdiffer)))
    print("new kernels (%d): %s" % (len(added), ", ".join(sorted({re.match(r"_ZN5mlkem\d+(\w+?)(?:I|E)", k).group(1) for k in added}))))
    for k in differ:
        print("INSTRUCTIONS DIFFER:", k)
    for k in rdiffer:
        print("RESOURCE USAGE DIFFERS:", k)
    return 1 if differ or rdiffer else 0


if __name__ == "__main__":
    sys.exit(main())
