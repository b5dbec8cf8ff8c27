"""Region moves (csrc/k_region.hip, option region_rounds) and the library's own node order (ctx->t_perm) on CRAFTED instances (util_cases
"region moves on crafted instances"): the tied_* and boundary instances of tests/test_gpu_mrf_crafted.py, whose dyadic-grid costs make
equal gains the rule and not the accident, and new ones for what those do not reach -- a region with 63 .. 129 candidates (the chunk loop
of rg_accumulate_kernel), a region of 700 faces spread over nine blocks, planted chains of gains, the edges of the definition.  Three
statements are compared as integers, without a tolerance: the kernels, the CPU oracle (end to end, under every parameter set) and
region_round_numpy, written from the rule text alone (round by round from the argmin start).  The same solves run through
Context.costs_upload_ordered with the table in the identity, the reversed and a random order: every rule defined on the caller's ids
(colouring keys, the ICM winner, region names, the label scatter, the adjacency renumbering) then goes through orig[], and the result
must still be the oracle's, which knows no order.

Which test fails for which rule: DESIGN.md section 6, "Region moves, tie by tie"; tests/test_oracle.py holds, per rule, an instance on
which the rule's inversion changes the labels (REGION_WITNESSES) -- that is what makes the comparisons here able to fail."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U
from util_cases import energy_numpy

pytestmark = pytest.mark.gpu

CASES = {**{n: b for n, b in U.crafted_cases().items() if n in ("tied1", "tied3", "tied15", "boundary")}, **U.region_cases()}
PARAMS = {**U.CRAFTED_PARAMS, **U.CRAFTED_REGION_PARAMS}
STAT_KEYS = ("energy_fixed", "cut_edges", "sweeps", "icm_iters", "unseen", "region_rounds", "region_moves")
ORDERED = [(n, p) for n in ("tied1", "tied3") for p in ("start", "start_icm", "defaults6", "icm_only", "best_tie", "s30")] + [("chain", "start"), ("hub65_w64_aligned", "start")]
LARGER = "large_moves"          # 2100 nodes, more than any instance of ORDERED: its solve leaves the region scratch of a larger graph behind
_oracle_cache = {}


@pytest.fixture(scope="module")
def ctx():
    c = M.Context(0)
    yield c
    c.close()


def _csr(case):
    return O.CsrNp(len(case.col_ptr) - 1, case.n_views, case.col_ptr, case.view_id, case.cost)


def _table(case):
    return M.viewsel.DataCosts(len(case.col_ptr) - 1, case.n_views, case.col_ptr, case.view_id, case.cost)


def _oracle(name, pname):
    """the oracle's (labels, stats) of an (instance, parameter set): computed once, shared by the tests, never written to"""
    if (name, pname) not in _oracle_cache:
        case = CASES[name]()
        labels, st = O.view_selection(_csr(case), case.adj_ptr, case.adj, O.default_mrf_params(**PARAMS[pname]))
        labels.setflags(write=False)
        _oracle_cache[(name, pname)] = (labels, st)
    return _oracle_cache[(name, pname)]


def _solve_and_compare(c, name, pname, what=""):
    case = CASES[name]()
    lo, so = _oracle(name, pname)
    lg, sg = c.view_selection(case.adj_ptr, case.adj, M.viewsel.default_mrf_params(**PARAMS[pname]))
    got, want = [sg[k] for k in STAT_KEYS], [so[k] for k in STAT_KEYS]
    diff = np.nonzero(lg != lo)[0]
    assert len(diff) == 0, "%s %s %s: %d labels differ from the oracle's, first at node %d: %d for %d; stats %s for %s" % (
        name, pname, what, len(diff), diff[0], lg[diff[0]], lo[diff[0]], got, want)
    assert got == want, "%s %s %s: %s = %s, the oracle's %s" % (name, pname, what, STAT_KEYS, got, want)
    assert energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, lg) == (sg["energy_fixed"], sg["cut_edges"])
    return lg, sg


@pytest.mark.parametrize("pname", list(U.CRAFTED_REGION_PARAMS))
@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end(ctx, name, pname):
    """labels, energy, cut edges, sweeps, ICM iterations, unseen faces, region rounds and region moves equal the oracle's; the energy is
    that of the labels, and not above the same solve's without region rounds"""
    case = CASES[name]()
    ctx.costs_upload(_table(case))
    lg, sg = _solve_and_compare(ctx, name, pname)
    l0, s0 = ctx.view_selection(case.adj_ptr, case.adj, M.viewsel.default_mrf_params(**{**PARAMS[pname], "region_rounds": 0}))
    assert (s0["region_rounds"], s0["region_moves"]) == (0, 0) and sg["energy_fixed"] <= s0["energy_fixed"]
    if pname == "start":
        assert np.array_equal(l0, U.argmin_labels(case)) and (sg["sweeps"], sg["icm_iters"]) == (0, 0)
    if name == "chain" and pname == "start":
        assert (sg["region_rounds"], sg["region_moves"]) == (2, 5)          # stops by itself, far below the 8 rounds allowed
    if name == "large_zero":
        assert (sg["region_rounds"], sg["region_moves"]) == (0, 0)
    if name in ("edges_no_cut", "edges_single"):
        assert (sg["region_rounds"], sg["region_moves"], sg["cut_edges"]) == (0, 0, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_every_round_equals_the_rule_text(ctx, name):
    """"start" with region_rounds = 1, 2, ..: the labels after EVERY round are those of region_round_numpy -- the third statement against
    the kernels directly -- and the statistics count its rounds and moves; one round more than it finds moves in changes nothing"""
    case = CASES[name]()
    rounds = U.region_rounds_numpy(case, U.argmin_labels(case), PARAMS["start"]["region_rounds"])
    e0 = energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, U.argmin_labels(case))[0]
    ctx.costs_upload(_table(case))
    moves = 0
    settled = len(rounds) < PARAMS["start"]["region_rounds"]       # the model met a round without a move (tied3 still moves in its eighth)
    for r, (lab, moved, _) in enumerate(rounds + (rounds[-1:] if settled else []), 1):
        done = min(r, len(rounds))
        if r <= len(rounds): moves += len(moved); e0 -= sum(g for _, g in moved.values())
        lg, sg = ctx.view_selection(case.adj_ptr, case.adj, M.viewsel.default_mrf_params(**{**PARAMS["start"], "region_rounds": r}))
        diff = np.nonzero(lg != lab)[0]
        assert len(diff) == 0, "%s: after round %d %d labels differ from the model's, first at node %d: %d for %d" % (name, done, len(diff), diff[0], lg[diff[0]], lab[diff[0]])
        assert (sg["region_rounds"], sg["region_moves"], sg["energy_fixed"]) == (done, moves, e0), "%s round %d" % (name, r)
    if not rounds:
        lg, sg = ctx.view_selection(case.adj_ptr, case.adj, M.viewsel.default_mrf_params(**PARAMS["start"]))
        assert np.array_equal(lg, U.argmin_labels(case)) and (sg["region_rounds"], sg["region_moves"], sg["energy_fixed"]) == (0, 0, e0)


@pytest.mark.parametrize("order_name", ["identity", "reversed", "random"])
@pytest.mark.parametrize("name,pname", ORDERED, ids=["%s-%s" % np_ for np_ in ORDERED])
def test_table_orders(ctx, name, pname, order_name):
    """the table uploaded in a given order of its columns (the state a data-cost pass of the context leaves behind): whatever the order,
    labels and statistics are the oracle's, which knows no order -- a tie decided on positions where the rule says the caller's ids shows
    under the reversed and the random order.  Twice on one context, the second time behind the solve of a larger instance."""
    case = CASES[name]()
    F = len(case.col_ptr) - 1
    order = U.table_orders(F)[order_name]
    big = CASES[LARGER]()
    assert len(big.col_ptr) - 1 > F
    for turn in ("first", "behind a larger solve"):
        ctx.costs_upload_ordered(_table(case), order)
        assert np.array_equal(ctx.table_order(), order)
        _solve_and_compare(ctx, name, pname, "(%s order, %s)" % (order_name, turn))
        if turn == "first":
            ctx.costs_upload_ordered(_table(big), U.table_orders(len(big.col_ptr) - 1)["random"])
            _solve_and_compare(ctx, LARGER, "start", "(random order)")
    ctx.costs_upload(_table(case))
    assert ctx.table_order() is None


def test_a_refused_order_leaves_the_context_usable(ctx):
    """an order with a repeated id, or with an id that is no node, is refused with MVS_ERR_INVALID (status 1); the good call right after
    it works, and so does the solve"""
    name = "chain"
    case = CASES[name]()
    F = len(case.col_ptr) - 1
    ctx.costs_upload(_table(case))
    for bad in (np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 8], np.uint32), np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, F], np.uint32), np.array([0xFFFFFFFF] + list(range(1, F)), np.uint32)):
        with pytest.raises(M.MvsError) as e:
            ctx.costs_upload_ordered(_table(case), bad)
        assert e.value.status == 1
        assert ctx.table_order() is None                          # the refusal touched nothing: the plain table is still the active one
        _solve_and_compare(ctx, name, "start", "(behind a refused order)")
        ctx.costs_upload_ordered(_table(case), U.table_orders(F)["reversed"])
        assert np.array_equal(ctx.table_order(), U.table_orders(F)["reversed"])
        _solve_and_compare(ctx, name, "start", "(reversed order, behind a refused one)")
        ctx.costs_upload(_table(case))
