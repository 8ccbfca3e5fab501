"""float64 restatement of nsd_head_fit (include/nsd.h, session calibration): one full-batch epoch of the read-out LayerNorm -> fc.0 ->
RReLU -> dropout -> fc.3 on frozen pooled features with the soft-target loss, and E epochs of Adam on it.  Adam is tests/optim_ref.py's
(no clipping, constant schedule), the noise of an epoch comes from the oracle's counter streams, the loss follows the soft-target
convention of nsd_head_train_soft.  tests/test_head_fit_cpu.py pins it to torch autograd + torch.optim.Adam; the GPU tests compare the
kernel with it.  numpy, the oracle's streams and optim_ref only; nothing here calls the library."""
import numpy as np

from oracle import nsd_oracle as orc
from tests.optim_ref import ClippedAdam

TAIL = ("ln.weight", "ln.bias", "fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias")      # the state's order: flat order without attn
GROUPS = {"ln": ("ln.weight", "ln.bias"), "fc0": ("fc.0.weight", "fc.0.bias"), "fc3": ("fc.3.weight", "fc.3.bias")}
BITS = {"ln": 1, "fc0": 2, "fc3": 4}
LN_EPS = 1e-5


def tail_shapes(H, F, K):
    return {"ln.weight": (H,), "ln.bias": (H,), "fc.0.weight": (F, H), "fc.0.bias": (F,), "fc.3.weight": (K, F), "fc.3.bias": (K,)}


def tail_count(H, F, K):
    return 2 * H + F * H + F + K * F + K


def state_layout(H, F, K):
    """nsd_fit_layout: float offsets of m, v, the int64 epoch count (even) and the int32 status word, and the stride (a multiple of 4)"""
    pt = tail_count(H, F, K)
    epochs = (2 * pt + 1) & ~1
    status = epochs + 2
    return dict(m=0, v=pt, epochs=epochs, status=status, stride=(status + 1 + 3) & ~3)


def lds_bytes(N, H, F, K):
    """the workgroup's LDS need the header states for nsd_head_fit_path"""
    image = 2 * H + F * (H + 1) + F + K * (F | 1) + K
    return 4 * (N * (2 * H + F + K + 3) + image + tail_count(H, F, K) + 520)


def tail_vector(theta, H, F, K):
    return np.concatenate([np.asarray(theta[k], dtype=np.float64).reshape(-1) for k in TAIL])


def tail_dict(vec, H, F, K):
    out, o = {}, 0
    for k, shp in tail_shapes(H, F, K).items():
        n = int(np.prod(shp))
        out[k] = np.asarray(vec[o:o + n], dtype=np.float64).reshape(shp)
        o += n
    return out


def trained_index(train, H, F, K):
    """boolean [Pt]: the tail elements of the groups `train` names"""
    names = [t for g in train for t in GROUPS[g]]
    return np.concatenate([np.full(int(np.prod(shp)), k in names) for k, shp in tail_shapes(H, F, K).items()])


def epoch_masks(seed, base_stream, e, p_head, N, F):
    """RReLU slopes and head-dropout multipliers [N,F] of global epoch e (0-based): streams base_stream + 4e + {1, 2} (uint32 wrap), what
    nsd_train_masks writes for a batch of N trials"""
    base = (int(base_stream) + 4 * int(e)) & 0xFFFFFFFF
    return (orc.rrelu_noise(seed, (base + 1) & 0xFFFFFFFF, (N, F)).astype(np.float64),
            orc.dropout_mask(seed, (base + 2) & 0xFFFFFFFF, p_head, (N, F)).astype(np.float64))


def soft_ce(logits, q, scale):
    """per-trial loss = - sum_k q_k log softmax_k, dlogits = scale (s p - q)"""
    m = logits.max(-1, keepdims=True)
    logp = logits - (m + np.log(np.exp(logits - m).sum(-1, keepdims=True)))
    return -(q * logp).sum(-1), scale * (q.sum(-1, keepdims=True) * np.exp(logp) - q)


def epoch(theta, feats, targets, scale, slope=None, drop=None):
    """One epoch's evaluation in float64 -> (loss = scale * sum_n loss_n, gradients by tensor name, fc.0's pre-activations, logits).
    slope: None (the eval slope) or [N,F]; drop: None or multipliers [N,F]."""
    t = {k: np.asarray(theta[k], dtype=np.float64) for k in TAIL}
    x = np.asarray(feats, dtype=np.float64)
    q = np.asarray(targets, dtype=np.float64)
    N, H = x.shape
    mu = x.mean(-1, keepdims=True)
    xc = x - mu
    rstd = 1.0 / np.sqrt((xc * xc).mean(-1, keepdims=True) + LN_EPS)
    xhat = xc * rstd
    ln = xhat * t["ln.weight"] + t["ln.bias"]
    pre = ln @ t["fc.0.weight"].T + t["fc.0.bias"]
    s = np.full_like(pre, orc.rrelu_eval_slope()) if slope is None else np.asarray(slope, dtype=np.float64)
    dm = np.ones_like(pre) if drop is None else np.asarray(drop, dtype=np.float64)
    fac = np.where(pre >= 0, 1.0, s) * dm
    z = pre * fac
    logits = z @ t["fc.3.weight"].T + t["fc.3.bias"]
    per, dl = soft_ce(logits, q, scale)
    dpre = (dl @ t["fc.3.weight"]) * fac
    dln = dpre @ t["fc.0.weight"]
    g = {"fc.3.weight": dl.T @ z, "fc.3.bias": dl.sum(0), "fc.0.weight": dpre.T @ ln, "fc.0.bias": dpre.sum(0),
         "ln.weight": (dln * xhat).sum(0), "ln.bias": dln.sum(0)}
    return scale * float(per.sum()), g, pre, logits


class HeadFitRef:
    """State of one model in float64: the tail, Adam's moments over the trained elements, the global epoch count.
    fp32_fields: lr, betas, eps, weight decay as the fp32 fields of nsd_fit hold them and the gradient rounded to fp32 before Adam, as
    the kernel hands it over (False: everything in float64, for the comparison with torch)."""

    def __init__(self, theta, H, F, K, *, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, train=("ln", "fc0", "fc3"),
                 rng=None, fp32_fields=True, count=0, m=None, v=None):
        self.H, self.F, self.K = H, F, K
        self.idx = trained_index(train, H, F, K)
        self.vec = tail_vector(theta, H, F, K)
        self.opt = ClippedAdam(self.vec[self.idx], lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay,
                               fp32_fields=fp32_fields, step=count)
        if m is not None:
            self.opt.m = np.asarray(m, dtype=np.float64)[self.idx].copy()
            self.opt.v = np.asarray(v, dtype=np.float64)[self.idx].copy()
        self.rng, self.losses, self.last_grad, self.min_pre = rng, [], None, np.inf

    @property
    def count(self):
        return self.opt.s

    def theta(self):
        return tail_dict(self.vec, self.H, self.F, self.K)

    def moments(self):
        """(m, v) as full tail vectors, zero where nothing is trained"""
        m, v = np.zeros_like(self.vec), np.zeros_like(self.vec)
        m[self.idx], v[self.idx] = self.opt.m, self.opt.v
        return m, v

    def fit(self, feats, targets, scale, epochs, masks=None):
        """masks: None (self.rng decides: None -> eval slope, else dict(seed=, base_stream=, p_head=)), or a list of (slope, drop) per epoch"""
        N = np.asarray(feats).shape[0]
        for i in range(epochs):
            if masks is not None:
                slope, drop = masks[i]
            elif self.rng is not None:
                slope, drop = epoch_masks(self.rng["seed"], self.rng["base_stream"], self.count, self.rng["p_head"], N, self.F)
            else:
                slope = drop = None
            loss, g, pre, _ = epoch(self.theta(), feats, targets, scale, slope, drop)
            self.losses.append(loss)
            self.min_pre = min(self.min_pre, float(np.abs(pre).min()))
            self.last_grad = tail_vector(g, self.H, self.F, self.K)
            self.opt.step(self.last_grad[self.idx])
            self.vec[self.idx] = self.opt.p
        return np.asarray(self.losses[-epochs:])
