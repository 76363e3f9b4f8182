"""How long a gating match takes (kami_amd.search.Match / ks_match_run, and kami_native's kami::eval).

Part 1, in this process: the same two engines, games, nodes and seed, every game played to the end (early_stop off), as
    reference   threads 1, leaves_per_tree 1, pipeline 0: the reference's schedule, two blocking calls per round
    pooled      the recommended configuration (--threads / --leaves / --pipeline)
    beside      pooled, while a pipelined Pool plays on `current`
alternated --reps times.  leaves_per_tree > 1 changes the search (several leaves of a tree selected before any comes
back), so a row's games are only the reference row's games when its leaves_per_tree is 1; the evaluations are counted.
--sweep adds one run each of a few other configurations.

Part 2, kami_native (oracle/_ref/dropin, when built): one generation with `evaluate_threads: 0` (the reference's loop, the
baseline) and with `evaluate_threads: N`, alternated --reps times; a gate's wall time is this tool's clock between the
first and the last EVAL line of the program's output.

min / median / max of every row go to --out (default profiles/match_bench.txt)."""
import argparse
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=10)
ap.add_argument("--nodes", type=int, default=128)
ap.add_argument("--threads", type=int, default=5)
ap.add_argument("--leaves", type=int, default=1)
ap.add_argument("--pipeline", type=int, default=1)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--filters", type=int, default=64)
ap.add_argument("--residuals", type=int, default=6)
ap.add_argument("--sweep", action="store_true")
ap.add_argument("--no-native", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.txt"))
args = ap.parse_args()

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def spread(xs):
    return f"min {min(xs):8.3f}  median {statistics.median(xs):8.3f}  max {max(xs):8.3f}"


def part1():
    from kami_amd import NN, weights as W, search as S, _lib as L
    F, C, R = 30, args.filters, args.residuals

    def engine(seed, generation):
        nn = NN(8, 8, F, 4672, filters=C, residuals=R, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
        nn.load_weights(W.random_weights(F, C, R, seed=seed, peaky=5.0), generation)
        return nn

    cur, cand = engine(1, 0), engine(2, 1)
    common = dict(games=args.games, nodes=args.nodes, seed=1, target_pct=54, early_stop=False)
    rows = {"reference": dict(threads=1, leaves_per_tree=1, pipeline=0),
            "pooled": dict(threads=args.threads, leaves_per_tree=args.leaves, pipeline=args.pipeline)}
    rows["beside"] = rows["pooled"]
    say(f"# part 1: Match, {R}x{C} bf16, {args.games} games x {args.nodes} nodes, every game to the end; pooled = {rows['pooled']}")
    S.Match(cur, cand, **dict(common, games=2, nodes=16), threads=2).run()          # warm-up
    secs, rate, table = {k: [] for k in rows}, {k: [] for k in rows}, {}
    for rep in range(args.reps):
        for name, kw in rows.items():
            pool, over, t = None, threading.Event(), None
            if name == "beside":
                pool = S.Pool(cur, games=256, threads=4, nodes=64, leaves_per_tree=2, seed=9, pipeline=True, coalesce_target=256, coalesce_wait_us=80)

                def selfplay():
                    while not over.is_set():
                        pool.run(min_evals=200000, max_seconds=30.0)

                t = threading.Thread(target=selfplay)
                t.start()
                time.sleep(0.2)
            res = S.Match(cur, cand, **common, **kw).run()
            if pool is not None:
                over.set()
                t.join()
                pool_rate = pool.run(0, 0.0).evals_per_s
                pool.close()
            evals = res.evals_current + res.evals_candidate
            secs[name].append(res.seconds)
            rate[name].append(evals / res.seconds)
            same = table.setdefault(kw["leaves_per_tree"], res.games) == res.games
            say(f"rep {rep} {name:9s} {res.seconds:8.3f} s  {evals:8d} evals  {evals / res.seconds:10,.0f} evals/s  {res.batches:7d} engine calls  "
                f"score {res.score}/{res.games_counted} accepted {res.accepted}  same games as the first run with these leaves: {same}"
                + (f"  (pool meanwhile: {pool_rate:,.0f} leaf-evals/s)" if pool is not None else ""))
    for name in rows:
        say(f"{name:9s} seconds  {spread(secs[name])}   evals/s  min {min(rate[name]):10,.0f}  median {statistics.median(rate[name]):10,.0f}  max {max(rate[name]):10,.0f}")
    if args.sweep:
        say("# sweep: threads, leaves_per_tree, pipeline (one run each)")
        for th, lv, pl in ((1, 1, 1), (2, 1, 1), (5, 1, 1), (10, 1, 1), (10, 1, 2), (5, 2, 1), (5, 4, 1), (5, 4, 2), (10, 4, 1), (10, 8, 1)):
            res = S.Match(cur, cand, **common, threads=th, leaves_per_tree=lv, pipeline=pl).run()
            evals = res.evals_current + res.evals_candidate
            say(f"threads {th:2d} leaves {lv} pipeline {pl}: {res.seconds:8.3f} s  {evals:8d} evals  {evals / res.seconds:10,.0f} evals/s  score {res.score}/{res.games_counted}")
    cur.close()
    cand.close()


def native_gate(exe, workdir, ethreads):
    """One kami_native run up to the end of its first gate -> (seconds between first and last EVAL line, games counted)."""
    os.makedirs(workdir, exist_ok=True)
    opts = dict(filters=32, residuals=2, selfplay_batch=16, selfplay_nodes=16, inference_threads=2, training_threads=1,
                replaybuffer_size=128, rpb_train_pct=40, training_sample_pct=60, training_epochs=2, training_batchsize=8,
                training_mlr=5, evaluate_batch=8, evaluate_games=args.games, evaluate_nodes=args.nodes, evaluate_target_pct=50,
                evaluate_threads=ethreads, evaluate_leaves=args.leaves, model_path=os.path.join(workdir, "model.bin"), engine_dtype="bf16")
    with open(os.path.join(workdir, "options.yml"), "w") as f:
        f.write("".join(f"{k}: {v}\n" for k, v in opts.items()))
    env = dict(os.environ)
    lib = os.path.join(ROOT, "kami_amd")
    env["LD_LIBRARY_PATH"] = lib + (os.pathsep + env["LD_LIBRARY_PATH"] if env.get("LD_LIBRARY_PATH") else "")
    proc = subprocess.Popen([exe], cwd=workdir, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    stamps, verdict = [], threading.Event()

    def read():
        for line in iter(proc.stdout.readline, ""):
            if line.startswith("EVAL") and not verdict.is_set():
                stamps.append((time.perf_counter(), line.strip()))
            if "candidate accepted" in line or "candidate rejected" in line:
                verdict.set()

    t = threading.Thread(target=read, daemon=True)
    t.start()
    ok = verdict.wait(timeout=240)
    try:
        proc.stdin.write("quit\n")
        proc.stdin.flush()
        proc.wait(timeout=60)
    except Exception:
        proc.kill()
    t.join(timeout=10)
    if not ok or len(stamps) < 2:
        raise RuntimeError(f"kami_native (evaluate_threads {ethreads}) did not finish a gate: {stamps[-3:]}")
    return stamps[-1][0] - stamps[0][0], sum(" game " in s for _, s in stamps), stamps[-1][1]


def part2():
    exe = os.path.join(ROOT, "oracle", "_ref", "dropin", "kami_native")
    if not os.path.exists(exe):
        say("# part 2 skipped: oracle/_ref/dropin/kami_native is not built")
        return
    import tempfile
    say(f"# part 2: kami_native, 2x32 bf16, one gate of {args.games} games x {args.nodes} nodes at 50 %, evaluate_threads 0 (the reference's loop) "
        f"against {args.threads} (evaluate_leaves {args.leaves}); wall time first..last EVAL line; seconds per counted game beside it")
    secs = {0: [], args.threads: []}
    per_game = {0: [], args.threads: []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(args.reps):
            for n in secs:
                dt, counted, last = native_gate(exe, os.path.join(tmp, f"r{rep}_{n}"), n)
                secs[n].append(dt)
                per_game[n].append(dt / max(1, counted))
                say(f"rep {rep} evaluate_threads {n:2d}: {dt:8.3f} s  {counted:2d} games counted  | {last}")
    for n in secs:
        say(f"evaluate_threads {n:2d} seconds  {spread(secs[n])}   seconds per counted game  {spread(per_game[n])}")


part1()
if not args.no_native:
    part2()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
