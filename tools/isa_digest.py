#!/usr/bin/env python3
"""Per-kernel digest of the gfx950 machine code of the H = 48 kernel files (no GPU needed).

    tools/isa_digest.py --csrc neural-speech-decoding_amd/csrc --out /tmp/isa_pr.json
    tools/isa_digest.py --compare /tmp/isa_parent.json /tmp/isa_pr.json
    tools/isa_digest.py --census --csrc neural-speech-decoding_amd/csrc          (step bodies of the one- and two-trial H = 48 kernels)
    tools/isa_digest.py --csrc neural-speech-decoding_amd/csrc --files nsd_stream48 nsd_head --out /tmp/isa_head.json

Used on the eight H = 48 kernel files (the default), and through --files on nsd_stream48 and nsd_head (digest and --census alike: any
file of csrc/ that compiles on its own is taken as it is).

Each of the files is compiled device-only in three flavours (the Makefile's FLAGS, + -DNSD_PROFILE=1, + -DNSD_ABLATE_HOOKS=1),
unbundled and disassembled; per function symbol the digest is the sha256 of its instructions (raw encodings included, leading
addresses dropped), and per kernel the record of its code-object note (registers, spills, LDS, scratch, kernarg size).  Two builds of
one source give equal digests; the device ELF itself carries a per-build id and is not compared.

--census: the shipped flavour of the role-split kernels as assembly; per kernel, every stretch of instructions between two s_barrier
in text order is a step body of some role.  Bodies are grouped by what they hold (packed products, exponentials, matrix and
store instructions, and for the backward's helper waves 4x4x1 products, bf16 conversions, 32x32x16 tile products and LDS-DMA requests: the groups are named by that, not by role) and by whether control enters or leaves them (a label or a branch inside: a tested body), and each group prints
its instruction counts, the index of every `s_waitcnt lgkmcnt(0)`, of the first v_pk_fma_f32 / v_pk_mul_f32, of the first v_exp_f32 and
of every LDS write (the first ds_write_b32 of a chain body is h), with the instructions between the last v_fma_f32 and that write, and
per body the v_cndmask_b32 inside the quad reduction (between the last packed product and the first exponential / last DPP add).
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


CENSUS_FILES = ["nsd_lstm2_fwd48", "nsd_lstm2_bwd48", "nsd_lstm2_multi_fwd48", "nsd_lstm2_multi_bwd48"]


def role_of(ops):
    n = lambda *pre: sum(o.startswith(pre) for o in ops)
    pk, ex, mf = n("v_pk_fma_f32", "v_pk_mul_f32"), n("v_exp_f32"), n("v_mfma")
    # named by content, not by role: which role of a kernel a group is follows from the kernel's source (forward: 28 packed products +
    # exponentials = layer 0, 24 + exponentials = layer 1, 24 alone = projection, 16-byte stores alone = saver; backward: 24 alone =
    # the recurrences)
    # the backward's helper waves, by what only they hold: the loader its LDS-DMA requests, the x1 waves the 4x4x1 products of the
    # four-step hand-off (with exponentials: a wave that also prepares a layer's factors; a prep step between two hand-offs is
    # "exponentials, no products"), the dW waves the bf16 conversions of their duty and the 32x32x16 tiles
    cv, m4, m32 = n("v_cvt_pk_bf16_f32"), n("v_mfma_f32_4x4x1"), n("v_mfma_f32_32x32x16")
    if n("global_load_lds"):
        return "LDS-DMA"
    if m4:
        return f"{m4} 4x4x1 products" + (" + exponentials" if ex else "")
    if cv or m32:
        return " + ".join(x for x in (f"{cv} bf16 conversions" if cv else "", f"{m32} 32x32x16 tile products" if m32 else "") if x)
    if mf:
        return "matrix instructions"
    if pk and ex:
        return f"{pk} packed products + exponentials"
    if pk:
        return f"{pk} packed products"
    if n("global_store_dwordx4") and not ex:
        return "16-byte stores, no products"
    if ex:
        return "exponentials, no products"
    return None


def census(csrc, files):
    flags = make_flags(csrc)
    for name in files:
        asm = subprocess.run([f"{ROCM}/bin/hipcc", *flags, "--cuda-device-only", "-S", name + ".hip", "-o", "-"], check=True,
                             capture_output=True, text=True, cwd=os.path.abspath(csrc)).stdout
        kernel, body, groups, meta = None, None, {}, {}
        def close(kernel, groups, meta):
            if kernel is None:
                return
            print(f"\n{name} {kernel}\n    " + " ".join(f"{k}={v}" for k, v in sorted(meta.items())))
            for (role, tested), g in sorted(groups.items()):
                c = lambda key: "..".join(str(v) for v in sorted({min(x[key] for x in g), max(x[key] for x in g)}))
                r = g[0]
                print(f"  {role}{' [tested: label or branch inside]' if tested else ''}: {len(g)} bodies\n"
                      f"    instr {c('n')} vector {c('vec')} packed {c('pk')} lds rd/wr {c('rd')}/{c('wr')} stores {c('st')} "
                      f"scalar incl. waits, nops, branches {c('sc')} (branches {c('br')})\n"
                      f"    per body, instr/scalar: {' '.join(str(x['n']) + '/' + str(x['sc']) for x in g)}\n"
                      f"    first body: lgkmcnt(0) at {r['w0']} | first product at {r['p0']} | first v_exp_f32 at {r['e0']} | lds writes at {r['wi']}"
                      f" | between the last v_fma_f32 and the first write: {r['gap']}"
                      f" | selects in the quad reduction: {' '.join(str(x['sel']) for x in g)}")
        for line in asm.splitlines():
            m = re.match(r"^(_Z\w+):", line)
            if m and "kernel" in m.group(1):
                close(kernel, groups, meta)
                kernel, body, groups, meta = m.group(1), None, {}, {}
                continue
            if kernel is None:
                continue
            km = re.match(r"^\s*; (NumVgprs|ScratchSize|LDSByteSize|NumSgprs|codeLenInByte)\s*[:=]\s*(\d+)", line)
            if km:
                meta[km.group(1)] = int(km.group(2))
                continue
            t = line.strip()
            if re.match(r"^\.LBB\w+:", t):
                if body is not None:
                    body["label"] = True
                continue
            if not t or t[0] in ".;" or line[0] not in "\t ":
                continue
            op = t.split()[0]
            if op == "s_endpgm":
                body = None
                continue
            if op == "s_barrier":
                if body is not None and body["ops"]:
                    ops = body["ops"]
                    role = role_of([o for o, _ in ops])
                    if role:
                        names = [o for o, _ in ops]
                        idx = lambda f: [i for i, (o, a) in enumerate(ops) if f(o, a)]
                        first = lambda l: l[0] if l else None
                        wr = idx(lambda o, a: o.startswith("ds_write"))
                        fm = idx(lambda o, a: o.startswith("v_fma_f32") or o.startswith("v_fmac_f32"))
                        lastf = max([i for i in fm if wr and i < wr[0]], default=None)
                        # selects inside the quad reduction: v_cndmask_b32 between the last packed product and the first exponential
                        # (a body without one: the last DPP add)
                        pks = idx(lambda o, a: o.startswith(("v_pk_fma_f32", "v_pk_mul_f32")))
                        red_end = None
                        if pks:
                            exps = [i for i in idx(lambda o, a: o.startswith("v_exp_f32")) if i > pks[-1]]
                            dpps = [i for i in idx(lambda o, a: o.startswith("v_add_f32_dpp")) if i > pks[-1]]
                            red_end = exps[0] if exps else (dpps[-1] if dpps else None)
                        sel = sum(o.startswith("v_cndmask_b32") for o in names[pks[-1]:red_end]) if red_end is not None else None
                        rec = {"n": len(ops), "vec": sum(o.startswith("v_") for o in names),
                               "pk": sum(o.startswith(("v_pk_fma_f32", "v_pk_mul_f32")) for o in names),
                               "rd": sum(o.startswith("ds_read") for o in names), "wr": len(wr),
                               "st": sum(o.startswith(("global_store", "buffer_store")) for o in names),
                               "sc": sum(o.startswith("s_") for o in names), "br": sum(o.startswith(("s_cbranch", "s_branch")) for o in names),
                               "w0": idx(lambda o, a: o == "s_waitcnt" and "lgkmcnt(0)" in a),
                               "p0": first(idx(lambda o, a: o.startswith(("v_pk_fma_f32", "v_pk_mul_f32")))),
                               "e0": first(idx(lambda o, a: o.startswith("v_exp_f32"))), "wi": wr, "sel": sel,
                               "gap": names[lastf + 1:wr[0]] if lastf is not None else None}
                        groups.setdefault((role, bool(body["label"] or rec["br"])), []).append(rec)
                body = {"ops": [], "label": False}
                continue
            if body is not None:
                body["ops"].append((op, t[len(op):]))
        close(kernel, groups, meta)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc")
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--files", nargs="*", default=FILES, help="files of csrc/ without .hip (default: the eight H = 48 kernel files)")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--subset", action="store_true", help="with --compare: only the objects the right side has")
    ap.add_argument("--table", action="store_true", help="with --compare: print every symbol, not only the differing ones")
    ap.add_argument("--census", action="store_true", help="step bodies (between two s_barrier) of the role-split kernels: instruction counts and wait positions")
    o = ap.parse_args()
    if o.census:
        census(o.csrc, o.files if o.files != FILES else CENSUS_FILES[:2])
        sys.exit(0)
    if o.compare:
        sys.exit(1 if compare(*o.compare, o.table, o.subset) else 0)
    digest(o.csrc, o.out, o.jobs, o.files)
