"""Weight averaging in the step tail, restated in numpy (the rule of include/nsd.h, nsd_avg): written once, run in float32 (the kernel's
bits: every operation below is one rounded numpy operation in the dtype) or in float64 (against torch.optim.swa_utils.AveragedModel)."""
import numpy as np

EMA, SWA = 1, 2


class AveragedWeights:
    def __init__(self, mode, decay=0.999, start_step=1, every=1, dtype=np.float32):
        assert mode in (EMA, SWA)
        self.mode, self.start_step, self.every, self.dtype = mode, int(start_step), int(every), np.dtype(dtype)
        self.w = self.dtype.type(1.0) - self.dtype.type(decay)            # fp32: 1.0f - decay, as the launch forms it once
        self.n = 0
        self.row = None

    def averages_at(self, s):
        return s >= self.start_step and (s - self.start_step) % self.every == 0

    def update(self, p, s, skipped=False):
        """p: the parameters after Adam step s (1-based).  Returns True where the step averaged."""
        if skipped or not self.averages_at(s):
            return False
        p = np.asarray(p, dtype=self.dtype)
        if self.n == 0:
            self.row = p.copy()
        else:
            d = p - self.row
            if self.mode == EMA:
                self.row = self.row + self.w * d
            else:
                self.row = self.row + d / self.dtype.type(self.n + 1)
        self.n += 1
        return True
