"""Time one tnp_sdf_train_grad call (the batch gradient of a training step)
for a list of net shapes: warm-up, then device events around each of REPS
calls, median and spread, one JSON line per (shape, batch size).

    python tools/train_step_time.py [--out FILE]

Shapes: (hidden, layers) 16 x 3 (train_net.h, for scale) and the wide 16 x 5,
32 x 3, 32 x 4 (train_wide.h), 4 levels (r 2..32, T 19), n = 1000 (the
reference's batch) and 65,536."""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tropical-nerf.pytorch_amd"))

SHAPES = [(16, 3), (16, 5), (32, 3), (32, 4)]
SIZES = [1000, 65536]
WARMUP, REPS = 20, 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from tropical import _hip
    from tropical.stanford.model import Net
    from tropical.stanford.sdf_train import BATCH_SIZE, CLAMP, EIK_W, SDFTrainer
    dev = torch.device("cuda", 0)
    lines = []
    for hidden, layers in SHAPES:
        torch.manual_seed(0)
        net = Net(num_layers=layers, num_hidden=hidden, levels=4, r_min=2, r_max=32, T=19)
        with torch.no_grad():
            net.enc.module.params.uniform_(-0.1, 0.1)
        net = net.to(dev)
        tr = SDFTrainer(net)
        for n in SIZES:
            g = torch.Generator().manual_seed(1)
            x = ((torch.rand(n, 3, generator=g) * 2 - 1) * 0.95).to(dev)
            gt = ((torch.rand(n, generator=g) * 2 - 1) * 0.3).to(dev)
            s, keep = net.tnp_desc()
            stream = ctypes.c_void_p(_hip.stream_ptr(dev))

            def call():
                _hip.check(_hip.lib().tnp_sdf_train_grad(
                    ctypes.byref(s), _hip.ptr(x), _hip.ptr(gt), n, CLAMP, EIK_W, BATCH_SIZE, _hip.ptr(tr.g_table),
                    _hip.ptr(tr.g_w), _hip.ptr(tr.stats), stream), "tnp_sdf_train_grad")

            for _ in range(WARMUP):
                call()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
            for a, b in ev:
                a.record()
                call()
                b.record()
            torch.cuda.synchronize()
            ms = sorted(a.elapsed_time(b) for a, b in ev)
            del keep
            lines.append(json.dumps(dict(hidden=hidden, layers=layers, levels=4, n=n, reps=REPS,
                                         median_ms=round(ms[REPS // 2], 5), p10_ms=round(ms[REPS // 10], 5),
                                         p90_ms=round(ms[9 * REPS // 10], 5))))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
