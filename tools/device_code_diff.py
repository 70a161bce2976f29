#!/usr/bin/env python3
"""Is the device code of two trees the same, function by function?  (no GPU needed)
    tools/device_code_diff.py PARENT_ROOT [THIS_ROOT] > profiles/rNN_device_code_parent_vs_X.txt
Every .hip of both trees' csrc is compiled to gfx950 assembly with the flags that `make -n -B` of that tree shows for it
(-c ... -o and -MMD -MP replaced by --offload-device-only -S).  A function is the text from its label to its .Lfunc_end
plus its .amdhsa_kernel block, comments stripped and the function's ordinal taken out of its local labels.  Functions
are matched by name across units, so one that moved to another file is still compared.  Also prints the two trees'
compile lines side by side.  Exit status 1 if any function differs or exists on one side only."""
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor


def compile_lines(root):
    """unit -> the compile command of `make -n -B` as a list, -MMD -MP dropped"""
    csrc = os.path.join(root, "objective-slam_amd", "csrc")
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, "ARCH=gfx950"], check=True, capture_output=True, text=True).stdout
    lines = {}
    for ln in out.splitlines():
        w = ln.split()
        if "-c" in w and "-shared" not in w:
            src = w[w.index("-c") + 1]
            lines[src] = [x for x in w if x not in ("-MMD", "-MP")]
    return csrc, lines


def flags_of(cmd):
    i = cmd.index("-c")
    return " ".join(cmd[:i] + [x for x in cmd[i + 2:] if x != "-o" and not x.endswith(".o")])


def assembly(csrc, cmd, tmp, tag):
    i = cmd.index("-c")
    src = cmd[i + 1]
    out = os.path.join(tmp, tag + "_" + src + ".s")
    c = cmd[:i] + ["--offload-device-only", "-S", src, "-o", out] + [x for x in cmd[i + 2:] if x != "-o" and not x.endswith(".o")]
    subprocess.run(c, check=True, cwd=csrc)
    return src, open(out).read()


def functions(text):
    """name -> normalised lines of the function and of its kernel descriptor"""
    lines = text.split("\n")
    names = re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M)
    fn = {}
    for name in names:
        body, on = [], None
        for ln in lines:
            if on is None and ln.startswith(name + ":"):
                on = "text"
            elif on is None and re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", ln):
                on = "desc"
            if on:
                s = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].rstrip())
                if on == "text" and re.match(r"\.Lfunc_end\d+:", s):
                    on = None
                    continue
                if s:
                    body.append(s)
                if on == "desc" and ".end_amdhsa_kernel" in s:
                    on = None
        fn[name] = body
    return fn


def tree(root, tmp, tag):
    csrc, lines = compile_lines(root)
    hips = sorted(s for s in lines if s.endswith(".hip"))
    with ThreadPoolExecutor(16) as ex:
        asm = dict(ex.map(lambda s: assembly(csrc, lines[s], tmp, tag), hips))
    fn = {}
    for src in hips:
        for name, body in functions(asm[src]).items():
            fn[name] = (src, body)
    return lines, fn


def main():
    parent = sys.argv[1]
    this = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        pl, pf = tree(parent, tmp, "parent")
        tl, tf = tree(this, tmp, "this")
    print("== compile lines (make -n -B) without -MMD -MP, the source and the object: the units that share a line")
    for tag, lines in (("parent", pl), ("this tree", tl)):
        by = {}
        for src, w in lines.items():
            by.setdefault(flags_of(w), []).append(src)
        for fl in sorted(by):
            print("%s: %s\n    %s" % (tag, fl, " ".join(sorted(by[fl]))))
    for src in sorted(set(pl) | set(tl)):
        if src not in pl or src not in tl:
            print("%-28s only in %s" % (src, "the parent" if src in pl else "this tree"))
        elif flags_of(pl[src]) != flags_of(tl[src]):
            print("%-28s DIFFERENT FLAGS" % src)
            bad += 1
    print("== functions: name, unit in the parent -> unit here, lines, verdict (the library's own kernels one by one,")
    print("== rocPRIM's instantiations as a count unless one differs)")
    lib_same = 0
    for name in sorted(set(pf) | set(tf)):
        if "rocprim" in name and name in pf and name in tf and pf[name][1] == tf[name][1]:
            lib_same += 1
            continue
        if name not in pf or name not in tf:
            print("%-90s only in %s (%s)" % (name, "the parent" if name in pf else "this tree", (pf.get(name) or tf.get(name))[0]))
            bad += 1
            continue
        (ps, pb), (ts, tb) = pf[name], tf[name]
        same = pb == tb
        bad += not same
        print("%-90s %s -> %s  %d lines  %s" % (name, ps, ts, len(pb), "same" if same else "DIFFERENT"))
        if not same:
            for d in list(difflib.unified_diff(pb, tb, "parent", "this", n=2, lineterm=""))[:200]:
                print("    " + d)
    print("== %d functions compared (%d of rocPRIM the same, not listed), %d differ or are unmatched" % (len(set(pf) | set(tf)), lib_same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
