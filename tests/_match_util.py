"""What tests/test_match.py (synthetic evaluators) and tests/test_gpu_match.py (real engines) share: the verdict of the
gating match restated from a result table, and the replay of a table's games through the rules."""
from kami_amd import search as S


def restate(rows, games, target_pct):
    """The verdict of evaluate.cpp:100-125 from a result table, in game-index order -> (accepted, score, counted)."""
    target = float((games * target_pct) // 100)             # integer division, evaluate.cpp:109
    score, counted = 0.0, 0
    for finished, candidate_white, result, _ in rows:
        if not finished:
            break
        score += result * (1.0 if candidate_white else -1.0) / 2 + 0.5
        counted += 1
        if score + (games - counted) < target:
            return False, score, counted
        if score >= target and counted < games:
            return True, score, counted
    return counted == games and score * 100 / games >= target_pct, score, counted


def check_legal_games(res, all_finished):
    """Replays every game: legal moves only, not over before the last move, over after it with the reported result."""
    for finished, _, result, moves in res.games:
        if all_finished:
            assert finished == 1
        env = S.Env()
        for a in moves:
            assert env.terminal()[0] is False
            env.push(a)                                     # raises on an illegal action
        if finished:
            assert len(moves) > 0 and env.terminal() == (True, result) and result in (-1.0, 0.0, 1.0)
        else:
            assert env.terminal()[0] is False
