"""Session calibration measured: one nsd_head_fit launch against the eager PyTorch loop a user has without it, and one experiment
on the recorded trials.  Writes profiles/session_calibration.md.

    python tools/session_calibration.py [--reps 30] [--eager-reps 5] [--commit <text>] [--out profiles/session_calibration.md]

Timing: every figure is GPU time between two HIP events recorded around the work on the current stream, after untimed repetitions of
the same shape; median and 10th / 90th percentile.  The two legs of a point alternate, in one process, on one GPU.  E = 200 epochs,
N = 12, 60, 240 trials, M = 1 and 5 models, the reference head (H = 48, F = 32, K = 3), eval-mode fit on the same features:
  launch   one nsd_head_fit call (state zeroed and parameters restored outside the timed window)
  E = 1    the same call with one epoch: the fixed cost of the launch, the staging and the write-back
  eager    per model, 200 times: LayerNorm, Linear, the leaky slope, Linear, soft cross-entropy, backward, torch.optim.Adam.step --
           fp32 tensors on the same card, the M models one after the other (the only route without the entry point)
Experiment: the 3-class recorded trials (tests/golden/recorded_trials_filtered.npz), per seed a random half trains a model with
Trainer, 4 trials per class of the other half calibrate it, the remainder is scored before and after.  Reported as measured.
"""
import argparse
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EPOCHS = 200
TRIALS, MODELS = (12, 60, 240), (1, 5)


def _pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def _fmt(v, unit=1.0):
    v = [x * unit for x in v]
    return f"{statistics.median(v):.1f} ({_pct(v, 0.1):.1f} .. {_pct(v, 0.9):.1f})"


def timing(a, torch, ops, dev, lines):
    spec = ops.ModelSpec()
    H, F, K = spec.H, spec.F, spec.K
    offs, shapes = spec.offsets(), spec.shapes()
    g = torch.Generator().manual_seed(0)
    slope = (0.125 + 1.0 / 3.0) / 2.0

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3                                   # microseconds

    def eager(theta, feats, q, N):
        """E epochs of one model: what a user writes today"""
        opt = torch.optim.Adam(theta.values(), lr=1e-3)
        for _ in range(EPOCHS):
            opt.zero_grad(set_to_none=True)
            ln = torch.nn.functional.layer_norm(feats, (H,), theta["ln.weight"], theta["ln.bias"], eps=1e-5)
            z = torch.nn.functional.leaky_relu(torch.nn.functional.linear(ln, theta["fc.0.weight"], theta["fc.0.bias"]), slope)
            logits = torch.nn.functional.linear(z, theta["fc.3.weight"], theta["fc.3.bias"])
            loss = -(q * torch.log_softmax(logits, -1)).sum() / N
            loss.backward()
            opt.step()
        return loss

    lines += ["| M | N | launch (E = 200), us | per epoch, us | E = 1, us | eager loop (E = 200), us | eager per epoch and model, us | eager / launch | final loss: launch, eager |",
              "|---|---|---|---|---|---|---|---|---|"]
    for M in MODELS:
        for N in TRIALS:
            p0 = ((torch.rand((M, spec.param_count), generator=g) - 0.5) * 0.4).to(dev)
            centres = torch.randn((K, H), generator=g)
            y = torch.arange(N) % K
            feats = (centres[y] + 0.5 * torch.randn((N, H), generator=g)).to(dev).contiguous()
            q = torch.eye(K)[y].to(dev).repeat(M, 1).contiguous()
            params, state = p0.clone(), ops.head_fit_state(spec, M, dev)
            losses = torch.empty((M, EPOCHS), device=dev)
            one = torch.empty((M, 1), device=dev)

            def restore():
                params.copy_(p0)
                state.zero_()

            def launch(E, out):
                ops.head_fit(spec, params, feats, q, state, epochs=E, lr=1e-3, loss_out=out)

            def eager_all():
                last = []
                for m in range(M):
                    theta = {k: p0[m, offs[k]:offs[k] + int(torch.Size(shapes[k]).numel())].clone().view(shapes[k]).requires_grad_(True)
                             for k in ("ln.weight", "ln.bias", "fc.0.weight", "fc.0.bias", "fc.3.weight", "fc.3.bias")}
                    last.append(eager(theta, feats, q[:N], N))
                return last

            t_fit, t_one, t_eager, last = [], [], [], None
            for r in range(a.warmup + a.reps):
                restore()
                t = timed(lambda: launch(EPOCHS, losses))
                restore()
                t1 = timed(lambda: launch(1, one))
                if r >= a.warmup:
                    t_fit.append(t)
                    t_one.append(t1)
                if r < 1 + a.eager_reps:                                   # one untimed eager repetition, then eager_reps timed ones
                    box = []
                    te = timed(lambda: box.append(eager_all()))
                    if r >= 1:
                        t_eager.append(te)
                    last = box[0]
            restore()
            launch(EPOCHS, losses)
            torch.cuda.synchronize()
            fit_last = float(losses[:, -1].mean())
            eager_last = float(torch.stack([v.detach() for v in last]).mean())
            mf, me = statistics.median(t_fit), statistics.median(t_eager)
            lines.append(f"| {M} | {N} | {_fmt(t_fit)} | {mf / EPOCHS:.2f} | {_fmt(t_one)} | {_fmt(t_eager)} | {me / EPOCHS / M:.1f} | "
                         f"{me / mf:.0f}x | {fit_last:.4f}, {eager_last:.4f} |")
            print(lines[-1], flush=True)


def experiment(a, torch, nsd_amd, dev, lines):
    import numpy as np
    from nsd_amd import data as D
    from nsd_amd.trainer import Trainer, save_reference_checkpoint
    ts = D.load_trials_npz(os.path.join(ROOT, "tests", "golden", "recorded_trials_filtered.npz"), x_key="x_filt")
    x_all, y_all = torch.from_numpy(ts.x).to(dev), torch.from_numpy(ts.y).to(dev)
    lines += ["", f"## Experiment on the recorded trials ({len(ts)} trials of 3 classes, 625 samples, host-filtered windows)", "",
              "| seed | train trials | calibration trials | scored trials | accuracy before | accuracy after | calibration loss before -> after |",
              "|---|---|---|---|---|---|---|"]
    tmp = tempfile.mkdtemp()
    for seed in range(a.seeds):
        perm = np.random.RandomState(seed).permutation(len(ts))
        tr, rest = np.sort(perm[:len(ts) // 2]), np.sort(perm[len(ts) // 2:])
        torch.manual_seed(seed)
        model = nsd_amd.EEG_LSTM(8, 48, 2, 3, 0.6).to(dev).train()
        trainer = Trainer(model, lr=1e-3, seed=seed + 1)
        tr_dev = torch.from_numpy(tr).to(dev)
        for epoch in range(a.train_epochs):
            for idx in D.epoch_batches(len(tr), 32, seed, epoch, drop_last=True):
                sel = tr_dev[torch.from_numpy(idx).to(dev)]
                trainer.step(x_all[sel].contiguous(), y_all[sel].contiguous(), global_batch=len(idx))
        model.eval()
        path = os.path.join(tmp, f"half_{seed}.pth")
        save_reference_checkpoint(model, path)
        pred = nsd_amd.SimplePredictor(path, 125, preprocess="identity")
        from nsd_amd.calibrate import split_calibration
        cal_l, held_l = split_calibration(ts.y[rest], 4, seed)
        cal, held = rest[cal_l], rest[held_l]

        def score():
            probs, _ = pred.predict_windows(ts.x[held].reshape(-1, ts.x.shape[-1]), ts.x.shape[1])
            return float((probs.argmax(1) == ts.y[held]).mean())

        acc0 = score()
        rep = pred.calibrate(ts.x[cal], ts.y[cal], epochs=100, lr=1e-3)
        acc1 = score()
        lines.append(f"| {seed} | {len(tr)} | {len(cal)} | {len(held)} | {acc0:.3f} | {acc1:.3f} | {rep['loss_before']:.3f} -> {rep['loss_after']:.3f} |")
        print(lines[-1], flush=True)


def main():
    import torch
    import nsd_amd
    from nsd_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager-reps", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--train-epochs", type=int, default=30)
    ap.add_argument("--commit", default="working tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_calibration.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("session_calibration: needs the MI355X (no GPU, no figures)")
    dev = torch.device("cuda:0")
    prop = torch.cuda.get_device_properties(dev)
    lines = ["# Session calibration: one nsd_head_fit launch against the eager PyTorch loop", "",
             f"Machine: {prop.name} ({prop.multi_processor_count} CUs), torch {torch.__version__}.  Commit: {a.commit}.", "",
             f"Method: `python tools/session_calibration.py --reps {a.reps} --eager-reps {a.eager_reps}` (its docstring describes the legs).  "
             f"GPU time between two HIP events, microseconds, median (10th .. 90th percentile) of {a.reps} repetitions after {a.warmup} "
             f"untimed ones ({a.eager_reps} after one for the eager loop).", ""]
    timing(a, torch, ops, dev, lines)
    experiment(a, torch, nsd_amd, dev, lines)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
