"""The code-object notes (private-segment sizes, register counts) of a kernel source of the library, for the tests that read them.
No GPU needed."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speech-decoding_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "llvm", "bin")
TARGET = "--targets=hip-amdgcn-amd-amdhsa--gfx950"


def device_elf(name, tmp):
    """llvm-readelf --notes of the gfx950 code object of csrc/<name>.hip: from the object the build left beside the source, or, where
    that is missing or older than the source or any header of the Makefile's HDRS, from a device-only compile with the Makefile's flags"""
    obj, elf = os.path.join(CSRC, name + ".o"), os.path.join(tmp, name + ".elf")
    run = lambda *c: subprocess.run(c, check=True, capture_output=True, text=True, cwd=CSRC)
    make = open(os.path.join(CSRC, "Makefile")).read()
    deps = [name + ".hip"] + re.search(r"^HDRS\s*:=\s*(.*)$", make, re.M).group(1).split()
    if name.startswith("nsd_lstm2_multi_"):                  # a model-batched twin includes the single-model file (the Makefile's rule)
        deps.append(name.replace("_multi_", "_") + ".hip")
    if os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(os.path.join(CSRC, d)) for d in deps):
        fat = os.path.join(tmp, name + ".fatbin")
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(tmp, name + ".copy.o"))
    else:
        flags = re.search(r"^FLAGS\s*\?=\s*(.*)$", make, re.M).group(1).replace("$(ARCH)", "gfx950")
        fat = os.path.join(tmp, name + ".co")
        run(os.path.join(ROCM, "bin", "hipcc"), *flags.split(), "--cuda-device-only", "-c", name + ".hip", "-o", fat)
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", TARGET, "--input=" + fat, "--output=" + elf)
    return run(os.path.join(LLVM, "llvm-readelf"), "--notes", elf).stdout
