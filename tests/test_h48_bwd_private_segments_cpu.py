"""Private segments (scratch) and registers of the H = 48 role-split backward kernels.  No GPU needed.

`lstm2_bwd48_kernel<1>` -- the benchmark's backward -- has no private segment: every dW duty is an instantiation of its own that
holds one lane base per LDS region (nsd_lstm2_bwd48.hip, dw16_role), where the all-duties-in-one body kept two dozen lane addresses
that hipcc spilled in front of the time loop and reloaded inside it and in the last-window block at the end of every trial
(88 bytes; profiles/h48_bwd_helper_loops.md).  The other instantiations of both files hold no more than they did before that change:
the two-trial kernels 20 bytes each, the model-batched one-trial kernel 88 (it has 28 now).  16 waves per workgroup leave 128 VGPRs.
The sizes are read from the code-object notes, as tests/test_h48_private_segments_cpu.py does."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speech-decoding_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "--targets=hip-amdgcn-amd-amdhsa--gfx950"

# private-segment bytes before the helper waves' duties were split (commit 196f97c), per kernel
BEFORE = {
    "nsd_lstm2_bwd48": {"lstm2_bwd48_kernelILi1E": 88, "lstm2_bwd48_kernelILi2E": 20},
    "nsd_lstm2_multi_bwd48": {"lstm2_bwd48_multi_kernelILi1E": 88, "lstm2_bwd48_multi_kernelILi2E": 20},
}


def _notes(name, tmp):
    obj, elf = os.path.join(CSRC, name + ".o"), os.path.join(tmp, name + ".elf")
    run = lambda *c: subprocess.run(c, check=True, capture_output=True, text=True, cwd=CSRC)
    src = os.path.join(CSRC, name + ".hip")
    deps = [src, os.path.join(CSRC, "nsd_lstm2_bwd48.hip"), os.path.join(CSRC, "nsd_ring_block.h")]
    if os.path.exists(obj) and all(os.path.getmtime(obj) >= os.path.getmtime(d) for d in deps):
        fat = os.path.join(tmp, name + ".fatbin")
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, name + ".copy.o"))
    else:
        flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).replace("$(ARCH)", "gfx950")
        fat = os.path.join(tmp, name + ".co")
        run(os.path.join(ROCM, "bin", "hipcc"), *flags.split(), "--cuda-device-only", "-c", name + ".hip", "-o", fat)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", TARGET, "--input=" + fat, "--output=" + elf)
    out = {}
    for block in re.split(r"^\s*- \.agpr_count:", run(os.path.join(LLVM, "llvm-readelf"), "--notes", elf).stdout, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", ".agpr_count:" + block, re.M))
        out[kv[".name"]] = {k: int(kv[k], 0) for k in (".private_segment_fixed_size", ".vgpr_count", ".agpr_count", ".vgpr_spill_count")}
    return out


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_backward_kernels_private_segments_and_registers(name, tmp_path):
    notes = _notes(name, str(tmp_path))
    kernels = {k: v for k, v in notes.items() if "lstm2_bwd48" in k}
    assert len(kernels) == 2, sorted(notes)
    for key, before in BEFORE[name].items():
        (sym, rec), = [(k, v) for k, v in kernels.items() if key in k]
        print(sym, rec)
        assert rec[".private_segment_fixed_size"] <= before, (sym, rec)
        assert rec[".vgpr_count"] + rec[".agpr_count"] <= 128, (sym, rec)      # 16 waves of 64 lanes per workgroup
    (sym, rec), = [(k, v) for k, v in kernels.items() if "lstm2_bwd48_kernelILi1E" in k] or [(None, None)]
    if sym is not None:                                                        # the single-model one-trial kernel: none at all
        assert rec[".private_segment_fixed_size"] == 0 and rec[".vgpr_spill_count"] == 0, (sym, rec)
