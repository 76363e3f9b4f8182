"""The gating match (ks_match_synthetic, include/kami_search.h) on the CPU: two hash evaluators that differ by a salt play
the loop of ks_match_run — every game is a legal game, the verdict is the reference's arithmetic, the table does not depend
on the schedule, and each tree's leaves reach the evaluator whose turn it is at the root.

The (salt_current, salt_candidate, seed) triples below were chosen by running match_synthetic (8 games, 16 nodes): their
points per game for the candidate are written next to them, which is what makes a case an early pass, an early fail or a
full-length verdict."""
import functools

import pytest

from kami_amd import search as S
from _match_util import check_legal_games, restate

GAMES, NODES = 8, 16


@functools.lru_cache(maxsize=None)
def play(salt_current, salt_candidate, seed, target_pct=50, threads=3, early_stop=False, candidate_white_first=True,
         leaves_per_tree=1, games=GAMES):
    """One match per distinct argument list for the whole module (the tests only read the result)."""
    return S.match_synthetic(salt_current, salt_candidate, games=games, threads=threads, nodes=NODES, leaves_per_tree=leaves_per_tree,
                             target_pct=target_pct, seed=seed, candidate_white_first=candidate_white_first, early_stop=early_stop)


def test_restatement_on_constructed_tables():
    """10 games at 54 %: target = (10 * 54) // 100 = 5 points.  Five points reached at game 9 pass (early); five points
    reached only at game 10 fail (50 % < 54 %)."""
    draw, win, loss = (1, 1, 0.0, []), (1, 1, 1.0, []), (1, 1, -1.0, [])
    at_nine = [draw] * 8 + [win, loss]                       # 4.0 after eight, 5.0 after nine
    assert restate(at_nine, 10, 54) == (True, 5.0, 9)
    at_ten = [draw] * 8 + [loss, win]                        # 4.0 after nine, 5.0 after ten
    assert restate(at_ten, 10, 54) == (False, 5.0, 10)
    assert restate([loss] * 10, 10, 54) == (False, 0.0, 6)   # 0 + 4 remaining < 5
    assert restate([(1, 0, -1.0, [])] * 10, 10, 54) == (True, 5.0, 5)      # black's wins count for a black candidate
    assert restate([win, (0, 1, 0.0, []), win], 3, 100) == (False, 1.0, 1)  # an unfinished row ends the replay


# candidate's points per game                                     verdict at target_pct
CASES = [
    (1, 2, 1, 50, "full"),      # .5 .5 .5 1 .5 0 .5 .5           4.0 only after game 8: 50 % >= 50 % passes
    (7, 8, 4, 50, "pass"),      # .5 .5 .5 .5 .5 1 .5 .5          4.0 after game 7
    (3, 4, 2, 75, "fail"),      # .5 .5 0 .5 .5 .5 .5 .5          target 6: 1.5 + 4 remaining after game 4
    (3, 4, 2, 50, "full"),      #                                 3.5 + 0 < 4 only after game 8
]


@pytest.mark.parametrize("sc,sd,seed,pct,kind", CASES)
def test_games_are_legal_and_the_verdict_is_the_restatement(sc, sd, seed, pct, kind):
    whole = play(sc, sd, seed, pct, early_stop=False)
    check_legal_games(whole, all_finished=True)
    want = restate(whole.games, GAMES, pct)
    assert (bool(whole.accepted), whole.score, whole.games_counted) == want and whole.skipped == 0
    assert {"full": want[2] == GAMES, "pass": want[0] and want[2] < GAMES, "fail": not want[0] and want[2] < GAMES}[kind]
    assert whole.candidate_wins + whole.current_wins + whole.draws == GAMES
    assert whole.moves == sum(len(g[3]) for g in whole.games) and whole.evals_current > 0 and whole.evals_candidate > 0
    # early_stop: the same verdict, and the games that finished are the same games
    cut = play(sc, sd, seed, pct, early_stop=True)
    check_legal_games(cut, all_finished=False)
    assert (bool(cut.accepted), cut.score, cut.games_counted) == want
    assert all(g[0] for g in cut.games[:want[2]])
    assert all(c == w for c, w in zip(cut.games, whole.games) if c[0])


def test_early_stop_cuts_the_other_games_off():
    """target_pct 0: the first counted game passes.  One worker, so what is cut off is the same on every run: game 0 is
    over after 410 plies, the longer games are not, and far fewer leaves were evaluated."""
    whole = play(7, 8, 4, 0, threads=1, early_stop=False)
    cut = play(7, 8, 4, 0, threads=1, early_stop=True)
    assert (cut.accepted, cut.score, cut.games_counted) == (whole.accepted, whole.score, whole.games_counted) == (1, 0.5, 1)
    assert cut.games[0] == whole.games[0] and any(not g[0] for g in cut.games)
    assert all(c == w for c, w in zip(cut.games, whole.games) if c[0])
    assert all(c[3] == w[3][:len(c[3])] for c, w in zip(cut.games, whole.games))        # a cut game is a prefix of the whole one
    assert cut.evals_current + cut.evals_candidate < whole.evals_current + whole.evals_candidate
    check_legal_games(cut, all_finished=False)


@pytest.mark.parametrize("leaves", [1, 3])
def test_table_does_not_depend_on_threads(leaves):
    one = play(7, 8, 4, threads=1, leaves_per_tree=leaves)
    three = play(7, 8, 4, threads=3, leaves_per_tree=leaves)
    assert one.games == three.games and (one.accepted, one.score, one.games_counted) == (three.accepted, three.score, three.games_counted)
    assert (one.evals_current, one.evals_candidate, one.moves) == (three.evals_current, three.evals_candidate, three.moves)
    check_legal_games(three, all_finished=True)


def test_leaves_per_tree_is_part_of_the_game():
    """(not a contract, a sanity check of the test above: the knob it holds fixed does change the search)"""
    assert play(7, 8, 4, threads=3, leaves_per_tree=1).games != play(7, 8, 4, threads=3, leaves_per_tree=3).games


def test_routing_swapped_models_and_colours_play_the_same_games():
    """match(A, B, white first) and match(B, A, black first) put the same evaluator on the same colour in every game."""
    ab = play(1, 2, 1, candidate_white_first=True)
    ba = play(2, 1, 1, candidate_white_first=False)
    assert [g[3] for g in ab.games] == [g[3] for g in ba.games] and [g[2] for g in ab.games] == [g[2] for g in ba.games]
    assert [g[1] for g in ab.games] == [1 - g[1] for g in ba.games] == [1, 0] * (GAMES // 2)
    assert ab.games_counted == ba.games_counted == GAMES            # (both verdicts are full-length: see CASES[0])
    assert ab.score + ba.score == GAMES
    assert (ab.evals_current, ab.evals_candidate) == (ba.evals_candidate, ba.evals_current)


def test_routing_a_model_against_itself():
    """match(A, A): the colour flag cannot matter to the moves.  With seed 4 the two decisive games (1 and 2) go to white once
    as candidate and once as current, so the score is games / 2 under either flag."""
    w = play(9, 9, 4, candidate_white_first=True)
    b = play(9, 9, 4, candidate_white_first=False)
    assert [g[3] for g in w.games] == [g[3] for g in b.games]
    assert w.score == b.score == GAMES / 2 and w.games_counted == b.games_counted == GAMES


def test_routing_both_evaluators_are_used():
    """A tree's leaves go to the model on move at its root: with a different candidate the games differ from A against
    A (a match that sent every leaf to `current` would play A against A)."""
    aa = play(1, 1, 1)
    ab = play(1, 2, 1)
    ba = play(2, 1, 1)
    assert any(x[3] != y[3] for x, y in zip(aa.games, ab.games))
    assert any(x[3] != y[3] for x, y in zip(aa.games, ba.games))
    bb = play(2, 2, 1)                                      # ... and one that sent every leaf to `candidate`, B against B
    assert any(x[3] != y[3] for x, y in zip(bb.games, ab.games))


def test_bad_arguments_are_refused():
    with pytest.raises(RuntimeError, match="nodes >= 2"):
        S.match_synthetic(1, 2, games=2, nodes=1)
    with pytest.raises(RuntimeError, match="pipeline"):
        S.match_synthetic(1, 2, games=2, nodes=4, pipeline=5)
