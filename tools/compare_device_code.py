#!/usr/bin/env python3
"""Per-kernel comparison of two device assembly files of one translation unit (hipcc <Makefile flags> -S --cuda-device-only), the
method of profiles/aggregate_refactor/README.md: kernels are matched by demangled name, bodies compared with the function's ordinal
taken out of the block labels.  One row per kernel: instructions, VGPRs, SGPRs, scratch bytes (private_segment_fixed_size), static
LDS bytes and the assembler's Occupancy before / after, whether the body is identical, and whether the conditions for a body that
differs hold (scratch no higher, occupancy no lower, static LDS equal).

    compare_device_code.py before.s after.s [--map 'regex=replacement' ...] > device_code.txt

--map rewrites the demangled names of the BEFORE file (e.g. to match an instance that lost template parameters)."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(0)
        tail = text[m.end():m.end() + 6000]
        if ".amdhsa_kernel " + name not in body:
            continue
        info = {}
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                         ("lds", r"; LDSByteSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")):
            info[key] = int(re.search(pat, tail).group(1))
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == info["scratch"], name
        norm = body.replace(name, "@K")
        norm = re.sub(r"BB\d+_", "BB_", norm)  # block labels (and the comments that name them) without the function's ordinal
        norm = re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", norm)
        norm = re.sub(r"[ \t]+;", " ;", norm)  # (the comment column moves with the label's length)
        norm = re.sub(r"\.L__unnamed_\d+|__hip_cuid_\w+", "@U", norm)
        info["insts"] = sum(1 for line in body.split("\n") if line.startswith("\t") and not line.lstrip().startswith((".", ";")))
        info["body"] = norm
        out[name] = info
    names = list(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    res = {}
    for n, d in zip(names, dem):
        d = d.replace("nqe::agg::(anonymous namespace)::", "").replace("nqe::agg::", "").replace("nqe::", "").replace("(anonymous namespace)::", "")
        res[re.sub(r"^void |\(.*$", "", d)] = out[n]
    return res


def main():
    args = sys.argv[1:]
    maps = []
    while "--map" in args:
        i = args.index("--map")
        pat, rep = args[i + 1].split("=", 1)
        maps.append((re.compile(pat), rep))
        del args[i:i + 2]
    before, after = kernels(args[0]), kernels(args[1])
    renamed = {}
    for name, k in before.items():
        new = name
        for pat, rep in maps:
            new = pat.sub(rep, new)
        renamed.setdefault(new, []).append((name, k))
    print(f"# kernels before {len(before)}, after {len(after)}; only before: {sorted(n for n in renamed if n not in after)}; only after: {sorted(n for n in after if n not in renamed)}")
    print("# kernel | instructions | VGPRs | SGPRs | scratch bytes | static LDS bytes | occupancy  (before -> after) | identical | conditions")
    bad = 0
    for name in sorted(after):
        a = after[name]
        if name not in renamed:
            print(f"{name} | new")
            continue
        bname, b = renamed[name][0]
        same = a["body"] == b["body"]
        ok = a["scratch"] <= b["scratch"] and a["occ"] >= b["occ"] and a["lds"] == b["lds"]
        bad += 0 if (same or ok) else 1
        cols = " | ".join(f"{b[k]} -> {a[k]}" for k in ("insts", "vgpr", "sgpr", "scratch", "lds", "occ"))
        note = "" if bname == name else f"  (before: {bname})"
        print(f"{name} | {cols} | {'yes' if same else 'no'} | {'-' if same else ('hold' if ok else 'BROKEN')}{note}")
    ident = sum(1 for n in after if n in renamed and after[n]["body"] == renamed[n][0][1]["body"])
    print(f"# identical {ident} of {len(after)}; bodies that differ and break a condition: {bad}")


if __name__ == "__main__":
    main()
