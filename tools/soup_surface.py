"""What the four tools/*_kernel_ms.py share: the import path, the synth64h
surface (the 64^3 hashed lattice after all 33 steps, as bench.finish_check)
as a polygon soup on the device, and the wall clock."""
import os
import statistics
import sys
import time

sys.path[:0] = [os.getcwd(), os.path.join(os.getcwd(), "tropical-nerf.pytorch_amd"),
                os.path.join(os.getcwd(), "tests")]
import torch  # noqa: E402

from golden_io import load  # noqa: E402
from helpers import product_net  # noqa: E402
from tropical._engine import engine_for  # noqa: E402

dev = torch.device("cuda", 0)


def synth64h_surface():
    """``(engine, vertices, offsets, indices)`` with the faces' rows cached."""
    eng = engine_for(product_net(load("synth64h"), dev))
    eng.lattice()
    eng.run_steps([])
    eng.surface()
    verts, _, _ = eng.export(edges=False)
    eng.faces()
    off, idx, _ = eng.polygons()
    return eng, verts, off, idx


def wall(fn, reps=5):
    """Median wall time of fn() in ms, stream-synchronised."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(dev)
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4)
