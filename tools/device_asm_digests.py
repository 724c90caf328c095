#!/usr/bin/env python3
"""Developer probe: one sha256 per device function of a tree, to show that code which was only moved compiles to the same
instructions.

usage: tools/device_asm_digests.py [tree, default this one] > digests.txt
       tools/device_asm_digests.py --diff before.txt after.txt
       tools/device_asm_digests.py --counts before_tree after_tree [unit ...]

Every .hip unit of the Makefile's DEV_SRCS is compiled for the device alone with the library's flags (plus
--cuda-device-only -S -cuid=cmp: a pinned unit id, so that two trees name their unit-local symbols alike), a second time
with EXACT_FLAGS where EXACT_SRCS lists it.  One line per function symbol:

    <flavour> <symbol> <sha256 of its instructions> <sha256 of its .amdhsa_kernel block, - for a device function>
    <next_free_vgpr> <private_segment_fixed_size> <unit>

Labels that carry the function's index in its unit (.LBB<n>_, .Lfunc_end<n>, .Ltmp<n>) are normalised first, since a
function that changes files changes its index, and the compiler's comments, which name blocks by it, are dropped.
--diff compares two such listings by (flavour, symbol) and ignores the unit; it prints what changed, appeared, went or
only changed files, and exits 1 if any digest or resource block differs.
--counts says WHAT moved where a digest did: the units (default: every .hip unit both trees' Makefiles list) are compiled
in both trees, and for every function of the first tree whose instructions or resource block differ in the second it
prints the instruction totals, whether the resource block is the same, and the mnemonics whose counts differ (+ more in
the second tree).  "none" means the same instructions in another order or with other operands.
"""
import collections
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LOCAL_LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp)\d+")


def make_var(text, name):
    m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M)
    return m.group(1).split() if m else []


def functions(listing):
    """symbol -> (instruction lines, .amdhsa_kernel block lines or None)"""
    code, hsa = {}, {}
    lines = listing.splitlines()
    is_function = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", listing, re.M))
    cur = None
    for line in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if cur is None and m and m.group(1) in is_function:
            cur = m.group(1)
            code[cur] = []
            continue
        if cur is not None:
            text = line.split(";")[0].rstrip()  # (the compiler's comments name blocks by the same index: "Header=BB2_3")
            if text:
                code[cur].append(LOCAL_LABEL.sub(r".\1", text))
            if re.match(r"^\.Lfunc_end\d+:", line):
                cur = None
    kernel = None
    for line in lines:
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernel = m.group(1)
            hsa[kernel] = []
        elif kernel is not None:
            if re.match(r"^\s*\.end_amdhsa_kernel", line):
                kernel = None
            else:
                hsa[kernel].append(line.strip())
    return code, hsa


def digest_unit(job):
    tree, unit, flavour, flags = job
    pkg = os.path.join(tree, "racer-tracer_amd")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.check_call(flags + ["--cuda-device-only", "-S", "-cuid=cmp", "-Wno-unused-command-line-argument", unit, "-o", out], cwd=pkg)
        with open(out) as f:
            code, hsa = functions(f.read())
    rows = []
    for sym, body in code.items():
        sha = hashlib.sha256("\n".join(body).encode()).hexdigest()
        block = hsa.get(sym)
        field = lambda key: next((l.split()[1] for l in block if l.startswith(key + " ")), "-") if block else "-"
        rows.append((flavour, sym, sha, hashlib.sha256("\n".join(block).encode()).hexdigest() if block is not None else "-",
                     field(".amdhsa_next_free_vgpr"), field(".amdhsa_private_segment_fixed_size"), unit))
    return rows


def unit_jobs(tree):
    """(unit, flavour, compiler command without the unit) of every .hip unit of a tree's Makefile"""
    with open(os.path.join(tree, "racer-tracer_amd", "Makefile")) as f:
        mk = f.read()
    hipcc = (make_var(mk, "HIPCC") or ["/opt/rocm/bin/hipcc"])[0]
    base = [hipcc, "--offload-arch=" + (make_var(mk, "ARCH") or ["gfx950"])[0]] + make_var(mk, "CXXFLAGS")
    exact = set(make_var(mk, "EXACT_SRCS"))
    jobs = []
    for unit in make_var(mk, "DEV_SRCS"):
        if unit.endswith(".hip"):
            jobs.append((unit, "fast", base))
            if unit in exact:
                jobs.append((unit, "exact", base + make_var(mk, "EXACT_FLAGS")))
    return jobs


def functions_of(job):
    tree, unit, flags = job
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.check_call(flags + ["--cuda-device-only", "-S", "-cuid=cmp", "-Wno-unused-command-line-argument", unit, "-o", out],
                              cwd=os.path.join(tree, "racer-tracer_amd"))
        with open(out) as f:
            return functions(f.read())


def counts(before, after, units):
    after_jobs = {(u, fl): flags for u, fl, flags in unit_jobs(after)}
    jobs = [(u, fl, flags) for u, fl, flags in unit_jobs(before) if (u, fl) in after_jobs and (not units or u in units)]
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        old = list(pool.map(functions_of, [(before, u, flags) for u, fl, flags in jobs]))
        new = list(pool.map(functions_of, [(after, u, after_jobs[(u, fl)]) for u, fl, flags in jobs]))
    same = moved = 0
    lines = []
    mnemonics = lambda body: collections.Counter(l.split()[0] for l in body if not l.endswith(":"))  # noqa: E731
    for (unit, flavour, _), (code_a, hsa_a), (code_b, hsa_b) in zip(jobs, old, new):
        for sym in sorted(code_a):
            if sym not in code_b:
                lines.append("%s %s: gone (%s)" % (flavour, sym, unit))
                continue
            block_same = hsa_a.get(sym) == hsa_b.get(sym)
            if code_a[sym] == code_b[sym] and block_same:
                same += 1
                continue
            moved += 1
            a, b = mnemonics(code_a[sym]), mnemonics(code_b[sym])
            delta = ", ".join("%s %+d" % (k, b[k] - a[k]) for k in sorted(set(a) | set(b)) if a[k] != b[k])
            lines.append("%s %s: %d -> %d instructions, resource block %s, mnemonic counts that differ: %s"
                         % (flavour, sym, sum(a.values()), sum(b.values()), "same" if block_same else "DIFFERS", delta or "none"))
    print("%d functions identical, %d moved" % (same, moved))
    print("\n".join(lines))
    return 0


def listing_of(tree):
    with open(os.path.join(tree, "racer-tracer_amd", "Makefile")) as f:
        mk = f.read()
    hipcc = (make_var(mk, "HIPCC") or ["/opt/rocm/bin/hipcc"])[0]
    base = [hipcc, "--offload-arch=" + (make_var(mk, "ARCH") or ["gfx950"])[0]] + make_var(mk, "CXXFLAGS")
    exact = set(make_var(mk, "EXACT_SRCS"))
    jobs = []
    for unit in make_var(mk, "DEV_SRCS"):
        if not unit.endswith(".hip"):
            continue
        jobs.append((tree, unit, "fast", base))
        if unit in exact:
            jobs.append((tree, unit, "exact", base + make_var(mk, "EXACT_FLAGS")))
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        rows = [r for unit_rows in pool.map(digest_unit, jobs) for r in unit_rows]
    return sorted(rows)


def read_listing(path):
    table = {}
    with open(path) as f:
        for line in f:
            w = line.split()
            if len(w) == 7:
                table[(w[0], w[1])] = w[2:]
    return table


def diff(before, after):
    a, b = read_listing(before), read_listing(after)
    changed = 0
    for key in sorted(set(a) | set(b)):
        if key not in b:
            print("gone     %s %s (%s)" % (key + (a[key][4],)))
        elif key not in a:
            print("new      %s %s (%s)" % (key + (b[key][4],)))
        elif a[key][:4] != b[key][:4]:
            what = "code" if a[key][0] != b[key][0] else "resources"
            print("changed  %s %s: %s; vgpr %s -> %s, scratch %s -> %s (%s -> %s)"
                  % (key + (what, a[key][2], b[key][2], a[key][3], b[key][3], a[key][4], b[key][4])))
        else:
            if a[key][4] != b[key][4]:
                print("moved    %s %s: %s -> %s, same digest" % (key + (a[key][4], b[key][4])))
            continue
        changed += 1
    print("%d of %d symbols differ" % (changed, len(set(a) | set(b))))
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    if len(sys.argv) >= 4 and sys.argv[1] == "--counts":
        sys.exit(counts(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]), sys.argv[4:]))
    tree = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for row in listing_of(tree):
        print(" ".join(row))
