"""The gating match on real engines (kami_amd.search.Match -> ks_match_run): legal games, the reference's verdict, a table
that does not depend on the schedule or on who else uses the engine, leaves routed to the model on move at the root, and
the two places the match is used from — cycle.generation(gate=...) and kami_native's "evaluate_threads".

Nets: F=30, C=32, R=1, bf16, KH_VALUE_PER_SAMPLE0, W.random_weights(seed 11 / 12, peaky=5.0); 8 games of 16 nodes unless a
test says otherwise.  A match is skipped unless the candidate's generation is the higher one, so each parameter set lives
in two engines: generation 0 (to be `current`) and generation 1 (to be `candidate`)."""
import functools
import threading

import numpy as np
import pytest

from kami_amd import NN, _lib as L, weights as W
from _match_util import check_legal_games, restate

pytestmark = pytest.mark.gpu

F, C, R = 30, 32, 1
GAMES, NODES = 8, 16
SEED_A, SEED_B = 11, 12


def engine(wseed, generation, dtype="bf16", filters=C, value_mode=L.KH_VALUE_PER_SAMPLE0, load=True):
    nn = NN(8, 8, F, 4672, filters=filters, residuals=R, dtype=dtype, value_mode=value_mode)
    if load:
        nn.load_weights(W.random_weights(F, filters, R, seed=wseed, peaky=5.0), generation)
    return nn


@functools.lru_cache(maxsize=None)
def shared_engine(wseed, generation):
    return engine(wseed, generation)


@functools.lru_cache(maxsize=None)
def play(cur_seed, cand_seed, leaves=1, threads=3, pipeline=1, early_stop=False, candidate_white_first=True, target_pct=50,
         seed=1):
    """One match per distinct argument list for the whole module (the tests only read the result)."""
    from kami_amd import search as S
    return S.Match(shared_engine(cur_seed, 0), shared_engine(cand_seed, 1), games=GAMES, threads=threads, nodes=NODES,
                   leaves_per_tree=leaves, target_pct=target_pct, seed=seed, candidate_white_first=candidate_white_first,
                   pipeline=pipeline, early_stop=early_stop).run()


def verdict(res):
    return bool(res.accepted), res.score, res.games_counted


def moves(res):
    return [g[3] for g in res.games]


def points(res):
    return sum(result * (1 if white else -1) / 2 + 0.5 for _, white, result, _ in res.games)


@pytest.mark.parametrize("leaves", [1, 3])
def test_games_are_legal_and_the_verdict_is_the_restatement(leaves):
    whole = play(SEED_A, SEED_B, leaves)
    check_legal_games(whole, all_finished=True)
    assert verdict(whole) == restate(whole.games, GAMES, 50) and whole.skipped == 0
    assert whole.candidate_wins + whole.current_wins + whole.draws == GAMES
    cut = play(SEED_A, SEED_B, leaves, early_stop=True)
    check_legal_games(cut, all_finished=False)
    assert verdict(cut) == verdict(whole)
    assert all(g[0] for g in cut.games[:cut.games_counted])
    assert all(c == w for c, w in zip(cut.games, whole.games) if c[0])
    for pct in (0, 101):                  # the same table under other targets: the first game passes / nothing can
        res = play(SEED_A, SEED_B, leaves, early_stop=True, target_pct=pct)
        assert verdict(res) == restate(whole.games, GAMES, pct) and all(c == w for c, w in zip(res.games, whole.games) if c[0])


@pytest.mark.parametrize("leaves", [1, 3])
def test_routing_by_symmetry(leaves):
    ab = play(SEED_A, SEED_B, leaves, candidate_white_first=True)
    ba = play(SEED_B, SEED_A, leaves, candidate_white_first=False)
    # the same evaluator on the same colour in every game: the same games, every point shared out once
    assert moves(ab) == moves(ba) and [g[2] for g in ab.games] == [g[2] for g in ba.games]
    assert [g[1] for g in ab.games] == [1 - g[1] for g in ba.games] == [1, 0] * (GAMES // 2)
    assert points(ab) + points(ba) == GAMES
    if ab.games_counted == ba.games_counted == GAMES:      # `score` stops at the verdict; two full-length verdicts saw every game
        assert ab.score + ba.score == GAMES
    assert (ab.evals_current, ab.evals_candidate) == (ba.evals_candidate, ba.evals_current)
    # a model against itself: the colour flag cannot matter to the moves, and the points split evenly over the two flags
    aw = play(SEED_A, SEED_A, leaves, candidate_white_first=True)
    ak = play(SEED_A, SEED_A, leaves, candidate_white_first=False)
    assert moves(aw) == moves(ak)
    assert points(aw) + points(ak) == GAMES
    if all(g[2] == 0.0 for g in aw.games):                 # no decisive game: games / 2 whichever colours the candidate had
        assert aw.score == ak.score == GAMES / 2
    # both evaluators are used: neither A against A nor B against B plays the games of A against B
    bb = play(SEED_B, SEED_B, leaves)
    assert any(x != y for x, y in zip(moves(aw), moves(ab))) and any(x != y for x, y in zip(moves(bb), moves(ab)))


@pytest.mark.parametrize("leaves", [1, 3])
def test_table_does_not_depend_on_the_schedule(leaves):
    ref = play(SEED_A, SEED_B, leaves, threads=1, pipeline=0)
    for threads, pipeline in ((3, 1), (3, 2)):
        res = play(SEED_A, SEED_B, leaves, threads=threads, pipeline=pipeline)
        assert res.games == ref.games and verdict(res) == verdict(ref)
        assert (res.evals_current, res.evals_candidate, res.moves) == (ref.evals_current, ref.evals_candidate, ref.moves)


def test_routing_by_the_engines_own_counters():
    from kami_amd import search as S
    cur, cand = engine(SEED_A, 0), engine(SEED_B, 1)          # engines nobody else uses
    before = cur.coalesce_stats()[1], cand.coalesce_stats()[1]
    res = S.Match(cur, cand, games=GAMES, nodes=NODES, threads=3, pipeline=1, early_stop=False, seed=1, target_pct=50).run()
    after = cur.coalesce_stats()[1], cand.coalesce_stats()[1]
    assert (after[0] - before[0], after[1] - before[1]) == (res.evals_current, res.evals_candidate)
    assert res.evals_current > 0 and res.evals_candidate > 0
    assert res.games == play(SEED_A, SEED_B).games


def test_beside_a_pool_on_the_current_engine():
    from kami_amd import search as S
    cur, cand = shared_engine(SEED_A, 0), shared_engine(SEED_B, 1)
    alone = play(SEED_A, SEED_B)
    pool = S.Pool(cur, games=32, threads=2, nodes=NODES, seed=3, pipeline=True)
    got, started, over = {"evals": 0}, threading.Event(), threading.Event()

    def selfplay():                                             # short runs back to back until the match is over
        try:
            while not over.is_set():
                started.set()
                got["evals"] = pool.run(min_evals=20000, max_seconds=10.0).evals
        except Exception as e:                                  # noqa: BLE001 (reported by the assert below)
            got["error"] = e
        started.set()

    t = threading.Thread(target=selfplay)
    t.start()
    try:
        started.wait()
        res = S.Match(cur, cand, games=GAMES, nodes=NODES, threads=3, pipeline=1, early_stop=False, seed=1, target_pct=50).run()
    finally:
        over.set()
        t.join()
        pool.close()
    assert "error" not in got and got["evals"] >= 20000
    assert res.games == alone.games and verdict(res) == verdict(alone)


def test_skipped_when_the_current_generation_is_not_older():
    from kami_amd import search as S
    for cand_generation in (0, 1):                             # equal, and older than current's
        cur, cand = engine(SEED_A, 1), engine(SEED_B, cand_generation)
        res = S.Match(cur, cand, games=4, nodes=12, threads=2).run()
        assert (res.skipped, res.accepted) == (1, 0)
        assert res.evals_current == res.evals_candidate == res.moves == 0 and not any(g[0] for g in res.games)


def test_a_failed_engine_call_leaves_nothing_behind():
    from kami_amd import search as S
    cand = engine(SEED_B, 1, load=False)
    # (`current` one generation behind whatever an engine without weights reports: the generation check of every round
    # must not hide the failure as a skip)
    cur = engine(SEED_A, cand.get_generation() - 1)
    match = S.Match(cur, cand, games=4, nodes=12, threads=2, early_stop=False, seed=2)
    with pytest.raises(RuntimeError, match="kh_load_weights"):
        match.run()
    env = S.Env()
    acts = np.array(env.actions(), np.int32)
    priors, value = cur.infer_legal(env.record(), np.array([0, len(acts)], np.int32), acts)
    assert abs(priors.sum() - 1.0) < 1e-3 and np.isfinite(value).all()
    cand.load_weights(W.random_weights(F, C, R, seed=SEED_B, peaky=5.0), cur.get_generation() + 1)
    res = match.run()
    check_legal_games(res, all_finished=True)
    assert verdict(res) == restate(res.games, 4, 54)


@pytest.mark.parametrize("dtype,filters,value_mode", [("f32", 16, L.KH_VALUE_PER_SAMPLE0), ("bf16", 96, L.KH_VALUE_PER_SAMPLE0),
                                                      ("bf16", 32, L.KH_VALUE_REFERENCE_FLAT)])
def test_other_engine_paths(dtype, filters, value_mode):
    """The f32 kernels, the per-layer kernels of a 96-filter net, and engines as kami::NN creates them (the determinism
    contract is not claimed for those: only that the games are games and the verdict is the table's)."""
    from kami_amd import search as S
    cur = engine(SEED_A, 0, dtype, filters, value_mode)
    cand = engine(SEED_B, 1, dtype, filters, value_mode)
    res = S.Match(cur, cand, games=4, nodes=12, threads=2, early_stop=False, seed=5).run()
    check_legal_games(res, all_finished=True)
    assert verdict(res) == restate(res.games, 4, 54)
    assert res.evals_current > 0 and res.evals_candidate > 0


def test_cycle_generation_with_a_gate(monkeypatch):
    """cycle.generation(gate=...) trains a clone, plays the match and installs the clone only if it was accepted; both
    branches are reached by target_pct 0 (the first counted game passes) and 101 (nothing can)."""
    from kami_amd import search as S, cycle
    from kami_amd.replay import ReplayBuffer
    nn = NN(8, 8, F, 4672, filters=32, residuals=2, dtype="bf16", value_mode=L.KH_VALUE_PER_SAMPLE0)
    nn.load_weights(W.random_weights(F, 32, 2, seed=21, peaky=3.0), 0)
    pool = S.Pool(nn, games=256, threads=4, nodes=16, seed=7)
    replay = ReplayBuffer(cycle.OBSIZE, cycle.PSIZE, 4096, seed=1)
    seen = {}

    class Spy(S.Match):                                        # what the candidate held when the match began
        def __init__(self, current, candidate, **kw):
            seen["current"], seen["weights"], seen["generation"] = current, candidate.get_weights(), candidate.get_generation()
            super().__init__(current, candidate, **kw)

    monkeypatch.setattr(S, "Match", Spy)
    kw = dict(play_evals=150000, play_seconds=60.0, epochs=2, batchsize=8, sample=256)

    def one(**gate):
        before = nn.get_weights(), nn.get_generation()
        out = cycle.generation(nn, pool, replay, gate=dict(games=4, nodes=12, threads=2, **gate), **kw)
        assert isinstance(out["accepted"], bool) and out["gate_games"] >= 1 and 0 <= out["gate_score"] <= out["gate_games"]
        assert seen["current"] is nn and seen["generation"] == before[1] + 1 and not np.array_equal(seen["weights"], before[0])
        if out["accepted"]:
            assert out["generation_after"] == out["generation_before"] + 1 == nn.get_generation()
            assert np.array_equal(nn.get_weights().view(np.uint32), seen["weights"].view(np.uint32))
        else:
            assert out["generation_after"] == out["generation_before"] == before[1] == nn.get_generation()
            assert np.array_equal(nn.get_weights().view(np.uint32), before[0].view(np.uint32))
        return out

    one()
    assert one(target_pct=0)["accepted"] is True
    assert one(target_pct=101)["accepted"] is False
    plain = cycle.generation(nn, pool, replay, **kw)
    assert not {"accepted", "gate_score", "gate_games"} & set(plain)
    assert plain["generation_after"] == plain["generation_before"] + 1


def test_kami_native_gates_on_the_worker_pool(tmp_path):
    """kami_native (the reference's kami.cpp on this repository's host side) with evaluate_threads: 2 — one generation; the
    gate prints the reference's lines from the match's table: the opening line, `game k of n` for k = 1, 2, ... in order,
    and one closing line."""
    import os, re, subprocess, time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "oracle", "_ref", "dropin", "kami_native")
    if not os.path.exists(exe):
        pytest.skip("drop-in binaries not built (needs the reference tree at build time)")
    opts = dict(filters=16, residuals=1, selfplay_batch=16, selfplay_nodes=16, inference_threads=2, training_threads=1,
                replaybuffer_size=128, rpb_train_pct=40, training_sample_pct=60, training_epochs=2, training_batchsize=8,
                training_mlr=5, evaluate_batch=8, evaluate_games=8, evaluate_nodes=8, evaluate_target_pct=0, evaluate_threads=2,
                evaluate_leaves=2, model_path=str(tmp_path / "model.bin"), engine_dtype="bf16")
    (tmp_path / "options.yml").write_text("".join(f"{k}: {v}\n" for k, v in opts.items()))
    env = dict(os.environ)
    lib = os.path.join(root, "kami_amd")
    env["LD_LIBRARY_PATH"] = lib + (os.pathsep + env["LD_LIBRARY_PATH"] if env.get("LD_LIBRARY_PATH") else "")
    proc = subprocess.Popen([exe], cwd=tmp_path, env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    lines = []
    t = threading.Thread(target=lambda: lines.extend(iter(proc.stdout.readline, "")), daemon=True)
    t.start()
    deadline = time.time() + 150
    done = False
    while time.time() < deadline and not done and proc.poll() is None:
        time.sleep(0.2)
        done = any("candidate accepted" in l or "candidate rejected" in l for l in lines)
    try:
        proc.stdin.write("quit\n"); proc.stdin.flush()
        proc.wait(timeout=60)
    except Exception:
        proc.kill()
    t.join(timeout=10)
    out = "".join(lines)
    assert done and proc.returncode == 0, out[-3000:]
    ev = [l.strip() for l in out.splitlines() if l.startswith("EVAL 0:")]
    first_gate = ev[:next(i for i, l in enumerate(ev) if "finished evaluating" in l or "aborting" in l or "skipping" in l) + 1]
    assert first_gate[0] == "EVAL 0: evaluating model generation 1 over 8 games", ev
    games = [re.match(r"EVAL 0: game (\d+) of 8 \[(-?[01])\]: score \d+%$", l) for l in first_gate[1:-1]]
    assert all(games) and [int(m.group(1)) for m in games] == list(range(1, len(games) + 1)) and len(games) >= 1, first_gate
    # target 0 %: the first counted game decides (evaluate.cpp:121-125)
    assert len(games) == 1 and re.match(r"EVAL 0: finished evaluating early: score >=\d+%, target 0$", first_gate[-1]), first_gate
    assert "evaluation failed" not in out and "candidate accepted: using new generation 1" in out, out[-3000:]
