"""No instantiation of the H = 48 role-split forward kernels has a private segment (scratch).  No GPU needed.

The model-batched one-trial forward is at its SGPR limit: one more live scalar in a chain role makes its entry block spill 16
kernel-argument SGPRs, which leaves a 68-byte private segment and makes every dispatch set up scratch (profiles/h48_step_census.md).
The sizes are read from the code-object notes of the objects the build leaves beside the sources; an object that is not there is
compiled device-only with the Makefile's flags."""
import re

import pytest

from tests.code_object import device_elf


@pytest.mark.parametrize("name", ["nsd_lstm2_fwd48", "nsd_lstm2_multi_fwd48"])
def test_forward_kernels_have_no_private_segment(name, tmp_path):
    notes = device_elf(name, str(tmp_path))
    sizes = {}
    for block in re.split(r"^\s*- \.agpr_count:", notes, flags=re.M)[1:]:
        kv = dict(re.findall(r"^\s*(\.[a-z_]+):\s*(.+?)\s*$", block, re.M))
        sizes[kv[".name"]] = int(kv[".private_segment_fixed_size"], 0)
    kernels = {k: v for k, v in sizes.items() if "lstm2_fwd48" in k}
    assert len(kernels) == 4, sorted(sizes)                  # <1>, <2>, <1, SOFT>, <2, SOFT>
    assert all(v == 0 for v in kernels.values()), kernels
