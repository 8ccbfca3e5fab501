#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 machine code of the H = 48 kernel files (no GPU needed).

    tools/isa_digest.py --csrc neural-speech-decoding_amd/csrc --out /tmp/isa_pr.json
    tools/isa_digest.py --compare /tmp/isa_parent.json /tmp/isa_pr.json

Each of the eight files is compiled device-only in three flavours (the Makefile's FLAGS, + -DNSD_PROFILE=1, + -DNSD_ABLATE_HOOKS=1),
unbundled and disassembled; per function symbol the digest is the sha256 of its instructions (raw encodings included, leading
addresses dropped), and per kernel the record of its code-object note (registers, spills, LDS, scratch, kernarg size).  Two builds of
one source give equal digests; the device ELF itself carries a per-build id and is not compared.
"""
import argparse
import concurrent.futures
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
FILES = ["nsd_lstm2_fwd48", "nsd_lstm2_fwd48x4", "nsd_lstm2_bwd48", "nsd_lstm2_bwd48x4",
         "nsd_lstm2_multi_fwd48", "nsd_lstm2_multi_fwd48x4", "nsd_lstm2_multi_bwd48", "nsd_lstm2_multi_bwd48x4"]
FLAVOURS = {"ship": [], "prof": ["-DNSD_PROFILE=1"], "ablh": ["-DNSD_ABLATE_HOOKS=1"]}
NOTE_KEYS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".vgpr_spill_count": "vgpr_spill",
             ".sgpr_spill_count": "sgpr_spill", ".group_segment_fixed_size": "lds", ".private_segment_fixed_size": "scratch",
             ".kernarg_segment_size": "kernarg", ".max_flat_workgroup_size": "wg"}


def make_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", "gfx950").split()


def one(job):
    csrc, name, flavour, flags, tmp = job
    stem = os.path.join(tmp, f"{flavour}_{name}")
    run = lambda *c: subprocess.run(c, check=True, capture_output=True, text=True, cwd=csrc).stdout
    run(f"{ROCM}/bin/hipcc", *flags, *FLAVOURS[flavour], "--cuda-device-only", "-c", name + ".hip", "-o", stem + ".co")
    run(f"{ROCM}/llvm/bin/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950",
        "--input=" + stem + ".co", "--output=" + stem + ".elf")
    dis = run(f"{ROCM}/llvm/bin/llvm-objdump", "-d", "--no-leading-addr", stem + ".elf")
    notes = run(f"{ROCM}/llvm/bin/llvm-readelf", "--notes", stem + ".elf")
    syms, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            # "<insn> // <address>: <encoding>"; the address goes, the encoding stays
            cur.append(re.sub(r"//\s*[0-9A-Fa-f]+:", "//", line.strip()))
    out = {s: {"sha256": hashlib.sha256("\n".join(b).encode()).hexdigest(), "insns": len(b)} for s, b in syms.items()}
    # a kernel's record in the note starts at `- .agpr_count:` (keys are sorted) and names itself in `.symbol: <kernel>.kd`
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        block = ".agpr_count:" + block
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sym = kv[".symbol"].strip("'\"")
        out.setdefault(sym[:-3] if sym.endswith(".kd") else sym, {})["note"] = {NOTE_KEYS[k]: int(kv[k], 0) for k in NOTE_KEYS}
    return f"{flavour}/{name}", out


def digest(csrc, out_path, jobs, files):
    flags = make_flags(csrc)
    with tempfile.TemporaryDirectory() as tmp:
        work = [(os.path.abspath(csrc), n, f, flags, tmp) for f in FLAVOURS for n in files]
        with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
            res = dict(ex.map(one, work))
    json.dump(res, open(out_path, "w"), indent=1, sort_keys=True)
    print(f"{out_path}: {sum(len(v) for v in res.values())} symbols in {len(res)} objects")


def compare(pa, pb, table, subset=False):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    for unit in sorted(set(a) | set(b) if not subset else set(b)):
        sa, sb = a.get(unit, {}), b.get(unit, {})
        if set(sa) != set(sb):
            bad += 1
            print(f"{unit}: symbol sets differ: only left {sorted(set(sa) - set(sb))}, only right {sorted(set(sb) - set(sa))}")
        for s in sorted(set(sa) & set(sb)):
            same = sa[s] == sb[s]
            bad += not same
            if table or not same:
                n = sa[s].get("note", {})
                res = " ".join(f"{k}={n[k]}" for k in ("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "lds", "scratch", "kernarg") if k in n)
                print(f"{unit} {s}\n    {sa[s].get('sha256', '-')[:16]} {sb[s].get('sha256', '-')[:16]} insns {sa[s].get('insns')} {sb[s].get('insns')}"
                      f" {'same' if same else 'DIFFERENT'}{'  ' + res if res else ''}")
                if not same and sa[s].get("note") != sb[s].get("note"):
                    print(f"    note left {sa[s].get('note')}\n    note right {sb[s].get('note')}")
    print("identical" if not bad else f"{bad} differences")
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc")
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--files", nargs="*", default=FILES, help="a subset of the eight files (without .hip)")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--subset", action="store_true", help="with --compare: only the objects the right side has")
    ap.add_argument("--table", action="store_true", help="with --compare: print every symbol, not only the differing ones")
    o = ap.parse_args()
    if o.compare:
        sys.exit(1 if compare(*o.compare, o.table, o.subset) else 0)
    digest(o.csrc, o.out, o.jobs, o.files)
