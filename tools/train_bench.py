"""SGD steps per second of kh_train (csrc/train.hip) at the reference's training batch sizes.
`whole call`: steps / wall time of one NN::train call of 2 epochs over n samples (what round 1 reported: includes the
call's fixed work — workspace, parameter upload, recording the step graph, installing the trained weights in the engine);
`marginal`: (t(4 epochs) - t(2 epochs)) / extra steps: what one more SGD step costs.

`python tools/train_bench.py records [alternations]`: the record path (kh_train_records) against the dense path (kh_train)
on the same samples, whole calls alternated within one process and one engine; see records_leg().

`python tools/train_bench.py optimizer [alternations]`: plain SGD calls alternated with calls that use every optimizer
option (momentum, Nesterov, L2 decay, clipping) in one process; see optimizer_leg()."""
import sys, os, time
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "/root/repo"))
import numpy as np
from kami_amd import NN, weights as W
rng = np.random.default_rng(0)


def random_records(n):
    """n valid records: a sparse random board each, 20-40 distinct actions with normalised shares, a value in [-1, 1]"""
    from kami_amd import _lib as L
    rec = np.zeros(n, L.RECORD_DTYPE)
    occ = rng.integers(0, 1 << 62, (n, 6), dtype=np.uint64) & rng.integers(0, 1 << 62, (n, 6), dtype=np.uint64)
    rec["board"]["piece_occ"] = occ
    rec["board"]["color_occ"][:, 0] = np.bitwise_or.reduce(occ, axis=1)
    rec["board"]["ply"] = rng.integers(0, 200, n)
    rec["board"]["ctm"] = rng.integers(0, 2, n)
    rec["value"] = rng.uniform(-1, 1, n)
    for i in range(n):
        k = int(rng.integers(20, 41))
        rec["nact"][i] = k
        rec["actions"][i, :k] = np.sort(rng.choice(4672, k, replace=False))
        v = rng.random(k).astype(np.float32)
        rec["visits"][i, :k] = v / v.sum()
    return rec


def records_leg(alternations=5):
    """Per shape: warm both paths up (graph recorded, buffers allocated), then alternate whole calls — records_to_arrays
    (the preparation a caller of the dense path needs), kh_train on its arrays, kh_train_records on the records — each
    from the same starting weights, timed with a host clock around the call (a call ends synchronised).  The dense
    kh_train is the baseline; min / median / max over the alternations."""
    import ctypes as C
    from kami_amd import _lib as L, cycle
    print(f"ring bytes per position: {L.RECORD_DTYPE.itemsize} compact, {(1920 + 4672 + 1) * 4} dense")
    for C_, R, tb, n, epochs in ((64, 6, 8, 307, 8), (64, 6, 64, 4096, 2), (128, 10, 32, 4096, 2)):
        nn = NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype="bf16")
        blob = W.random_weights(30, C_, R, seed=1)
        rec = random_records(n)
        ct = (L.Record * n).from_buffer_copy(rec.tobytes())
        t = {"prep": [], "dense": [], "records": []}
        for it in range(alternations + 1):                         # the first round is the warm-up
            t0 = time.perf_counter()
            x, p, v = cycle.records_to_arrays(nn, ct)
            t1 = time.perf_counter()
            nn.load_weights(blob, 0)
            t2 = time.perf_counter()
            ld = nn.train(x.reshape(n, 8, 8, 30), p, v, epochs=epochs, batchsize=tb)
            t3 = time.perf_counter()
            wd = nn.get_weights()
            nn.load_weights(blob, 0)
            t4 = time.perf_counter()
            lr = nn.train_records(rec, epochs=epochs, batchsize=tb)
            t5 = time.perf_counter()
            assert ld == lr and np.array_equal(wd.view(np.uint32), nn.get_weights().view(np.uint32))
            if it:
                t["prep"].append(t1 - t0); t["dense"].append(t3 - t2); t["records"].append(t5 - t4)
        steps = epochs * -(-n // tb)
        fmt = lambda a: "%8.2f /%8.2f /%8.2f ms" % (1e3 * min(a), 1e3 * float(np.median(a)), 1e3 * max(a))
        both = [a + b for a, b in zip(t["prep"], t["dense"])]
        print(f"{R}x{C_} F=30 batch {tb} n {n} epochs {epochs} ({steps} steps), min / median / max over {alternations} alternations:\n"
              f"  dense call alone        {fmt(t['dense'])}\n"
              f"  dense call + preparation{fmt(both)}\n"
              f"  record call             {fmt(t['records'])}\n"
              f"  host -> device per call: dense {steps * tb * 26372:,} B staged, records {n * 664 + epochs * n * 4:,} B", flush=True)
        nn.close()


def optimizer_leg(alternations=7):
    """Per shape two engines in one process, one trained with plain SGD and one with all four optimizer options (so
    neither re-records its step graph), calls alternated plain / optimizer from the same starting weights.  A step's
    cost is the difference of a 4-epoch and a 2-epoch call over the extra steps (the calls' fixed work cancels), host
    clock around the calls; min / median / max over the alternations after one warm-up round."""
    opts = dict(momentum=0.9, nesterov=True, weight_decay=1e-4, max_grad_norm=1.0)
    for C_, R, tb, n in ((64, 6, 8, 256), (256, 20, 32, 128)):
        blob = W.random_weights(30, C_, R, seed=1)
        x = rng.random((n, 8, 8, 30), dtype=np.float32)
        p = np.zeros((n, 4672), np.float32); p[np.arange(n), rng.integers(0, 4672, n)] = 1.0
        v = rng.choice(np.array([-1, 0, 1], np.float32), n)
        legs = {"plain": (NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype="bf16"), {}),
                "optimizer": (NN(8, 8, 30, 4672, filters=C_, residuals=R, dtype="bf16"), opts)}
        per_step = {k: [] for k in legs}
        extra = 2 * (n // tb)
        for it in range(alternations + 1):                         # the first round is the warm-up
            for name, (nn, kw) in legs.items():
                dt = []
                for epochs in (2, 4):
                    nn.load_weights(blob, 0)
                    t0 = time.perf_counter()
                    nn.train(x, p, v, epochs=epochs, batchsize=tb, **kw)
                    dt.append(time.perf_counter() - t0)
                if it:
                    per_step[name].append((dt[1] - dt[0]) / extra)
        norms = legs["optimizer"][0].last_grad_norms()
        fmt = lambda a: "%7.3f /%7.3f /%7.3f ms" % (1e3 * min(a), 1e3 * float(np.median(a)), 1e3 * max(a))
        print(f"{R}x{C_} F=30 batch {tb} n {n}: per step, min / median / max over {alternations} alternations "
              f"({blob.size:,} parameters; {int((norms > opts['max_grad_norm']).sum())} of {norms.size} steps of the last call clipped):\n"
              f"  plain SGD     {fmt(per_step['plain'])}\n"
              f"  all options   {fmt(per_step['optimizer'])}", flush=True)
        for nn, _ in legs.values():
            nn.close()


if len(sys.argv) > 1 and sys.argv[1] == "optimizer":
    optimizer_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 7)
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "records":
    records_leg(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    sys.exit(0)

CASES = ((30, 64, 6, 8, 256), (30, 64, 6, 64, 1024), (30, 256, 2, 8, 128), (30, 128, 10, 32, 256), (30, 256, 20, 32, 128), (30, 256, 20, 64, 256))
for F, C, R, tb, n in CASES:
    nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16")
    nn.load_weights(W.random_weights(F, C, R, seed=1), 0)
    x = rng.random((n, 8, 8, F), dtype=np.float32)
    p = np.zeros((n, 4672), np.float32); p[np.arange(n), rng.integers(0, 4672, n)] = 1.0
    v = rng.choice(np.array([-1, 0, 1], np.float32), n)
    nn.train(x[:tb], p[:tb], v[:tb], epochs=1, batchsize=tb)          # warm-up
    t0 = time.perf_counter()
    first, last = nn.train(x, p, v, epochs=2, batchsize=tb)
    dt = time.perf_counter() - t0
    steps = 2 * (n // tb)
    t0 = time.perf_counter()
    nn.train(x, p, v, epochs=4, batchsize=tb)
    dt4 = time.perf_counter() - t0
    marg = steps / max(dt4 - dt, 1e-9)
    print(f"{R}x{C} F={F} batch {tb}: whole call {steps / dt:7.1f} steps/s {steps * tb / dt:9.0f} samples/s | marginal {marg:7.1f} steps/s "
          f"({1e3 / marg:.2f} ms per step, fixed {1e3 * (dt - steps / marg):.1f} ms per call)  loss {first:.3f} -> {last:.3f}", flush=True)
