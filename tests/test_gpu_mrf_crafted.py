"""The MRF solver (csrc/k_mrf_setup.hip, k_mrf_sweep.hip, k_mrf_polish.hip) against the CPU oracle on CRAFTED instances (util_cases "crafted MRF instances"): tied costs, columns
exactly at the boundaries of the per-node routing, launches of one to three nodes, nodes without a neighbour in the model -- end to end
under parameter sets that each pin one tie rule, through every route of the set-up and the sweep loop, sweep by sweep against the
oracle's decode trace, and over three logical shards.  Every comparison is of integers or bit patterns: there is no tolerance.

Which test fails for which rule ("Solver, tie by tie"): the decode's first argmin -- every-sweep tests (the first
sweep and node that differ are named) and the end-to-end tests; the ICM candidate and winner rules -- end to end, "icm_only" above all,
and the sharded test across part boundaries; "keep the best sweep" -- test_end_to_end[tied1-best_tie] and the traced best labeling; the
stop rule's strict `<` -- the "plateau" parameters (40 sweeps).  Per class: tied* and boundary hold every class, range_c<class>_n<count>
exactly one, test_routes forces the generic kernel on everything."""
import numpy as np
import pytest

import mvs_texturing_amd as M
import oracle_py as O
import util_cases as U
from util_cases import energy_numpy

pytestmark = pytest.mark.gpu

CASES = U.crafted_cases()
BIG = [n for n in CASES if not n.startswith("range_")]
SMALL = [n for n in CASES if n.startswith("range_")]
STAT_KEYS = ("energy_fixed", "cut_edges", "sweeps", "icm_iters", "unseen")
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
        labels, st = O.view_selection(_csr(case), case.adj_ptr, case.adj, O.default_mrf_params(**U.CRAFTED_PARAMS[pname]))
        labels.setflags(write=False)
        _oracle_cache[(name, pname)] = (labels, st)
    return _oracle_cache[(name, pname)]


def _solve_and_compare(c, name, pname, what=""):
    case = CASES[name]()
    lo, so = _oracle(name, pname)
    lg, sg = c.view_selection(case.adj_ptr, case.adj, M.viewsel.default_mrf_params(**U.CRAFTED_PARAMS[pname]))
    got, want = [sg[k] for k in STAT_KEYS], [so[k] for k in STAT_KEYS]
    diff = np.nonzero(lg != lo)[0]
    assert len(diff) == 0, "%s %s %s: %d labels differ from the oracle's, first at node %d (class %d, K = %d): %d for %d; stats %s for %s" % (
        name, pname, what, len(diff), diff[0], U.node_classes_numpy(case.col_ptr, case.adj_ptr, case.adj)[diff[0]],
        case.col_ptr[diff[0] + 1] - case.col_ptr[diff[0]], lg[diff[0]], lo[diff[0]], got, want)
    assert got == want, "%s %s %s: (energy_fixed, cut_edges, sweeps, icm_iters, unseen) = %s, the oracle's %s" % (name, pname, what, got, want)
    return lg, sg


@pytest.mark.parametrize("pname", list(U.CRAFTED_PARAMS))
@pytest.mark.parametrize("name", BIG)
def test_end_to_end(ctx, name, pname):
    """labels, energy, cut edges, sweeps, ICM iterations and unseen faces equal the oracle's; the energy is that of the labels"""
    case = CASES[name]()
    ctx.costs_upload(_table(case))
    lg, sg = _solve_and_compare(ctx, name, pname)
    assert energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, lg) == (sg["energy_fixed"], sg["cut_edges"])
    if pname == "plateau":
        assert sg["sweeps"] == 40
    if pname == "icm_only":
        assert sg["sweeps"] == 0


@pytest.mark.parametrize("pname", list(U.CRAFTED_PARAMS))
@pytest.mark.parametrize("name", SMALL)
def test_ranges_of_a_few_nodes(ctx, name, pname):
    """every (colour, class) launch holds exactly `count` nodes: 1, 2, 3, and a block's node count - 1, + 0, + 1 -- under every parameter
    set ("best_tie": the undamped kernels alone; "icm_only", "window1": no sweep or very few)"""
    case = CASES[name]()
    ctx.costs_upload(_table(case))
    lg, sg = _solve_and_compare(ctx, name, pname)
    assert energy_numpy(case.col_ptr, case.view_id, case.cost, case.adj_ptr, case.adj, lg) == (sg["energy_fixed"], sg["cut_edges"])
    if pname == "plateau":
        assert sg["sweeps"] == 40
    if pname == "icm_only":
        assert sg["sweeps"] == 0
    cls = int(name.split("_")[1][1:])
    assert ctx.mrf_diagnostics()["generic_nodes"] == (len(case.col_ptr) - 1 if cls == 4 else 0)


@pytest.mark.parametrize("name", [n for n in BIG if n.startswith("tied")])
def test_routes(name):
    """the generic kernel for every node, direct launches instead of graph replay, the set-up from view lists instead of bitmaps, and
    a second solve on the same context: the same labels and statistics as the oracle's every way"""
    case = CASES[name]()
    for option in (None, "mrf_force_generic", "mrf_graph", "mrf_force_lists"):
        c = M.Context(0)
        try:
            if option: c.set_option(option, 0 if option == "mrf_graph" else 1)
            c.costs_upload(_table(case))
            _solve_and_compare(c, name, "s30", "(%s, first solve)" % option)
            _solve_and_compare(c, name, "s30", "(%s, second solve)" % option)
            d = c.mrf_diagnostics()
            if option == "mrf_force_generic": assert d["generic_nodes"] == len(case.col_ptr) - 1
            if option == "mrf_graph": assert d["graph_launches"] == 0
            if option == "mrf_force_lists": assert c.mrf_setup_tables()["bitmaps"] is False
            if option is None: assert d["graph_launches"] > 0 and c.mrf_setup_tables()["bitmaps"] is True
        finally:
            c.close()


def test_boundary_classes_are_routed_by_the_documented_rule(ctx):
    """the set-up's routing of `boundary` (its labels are test_end_to_end's): as many generic nodes and fast-node descriptors as the class
    rule, restated in numpy, gives"""
    case = CASES["boundary"]()
    cls = U.node_classes_numpy(case.col_ptr, case.adj_ptr, case.adj)
    ctx.costs_upload(_table(case))
    ctx.view_selection(case.adj_ptr, case.adj, M.viewsel.default_mrf_params(**U.CRAFTED_PARAMS["icm_only"]))
    assert ctx.mrf_diagnostics()["generic_nodes"] == int((cls == 4).sum())
    assert ctx.mrf_setup_tables()["desc"].shape[0] == int((cls != 4).sum())


# ---- every sweep: one context driven through the building blocks, decode and best labeling read back after each sweep

def _drive_sweeps(case, n_sweeps, pieces, device_step):
    """(lab[n, F], best[n, F], energy[n]) of n_sweeps sweeps on one context through the building-block entry points: per sweep every colour
    phase over `pieces` node ranges, the tracking energy, then the bookkeeping -- the device's own step (device_step) or the host's
    comparison + keep_best, as a sharded driver does it"""
    import torch
    import multigpu as G
    F = len(case.col_ptr) - 1
    dev = torch.device("cuda:0")
    c = M.Context(0)
    try:
        c.costs_upload(_table(case))
        tap, tad = torch.from_numpy(np.array(case.adj_ptr).view(np.int32)).to(dev), torch.from_numpy(np.array(case.adj).view(np.int32)).to(dev)
        params = M.viewsel.default_mrf_params(max_sweeps=n_sweeps, min_sweeps=n_sweeps)
        ops = G.GpuShardOps(c, tap, tad, params); ops.setup()
        n_phases = ops.n_phases()
        cuts = [(F * p) // pieces for p in range(pieces + 1)]
        idx = torch.arange(F, dtype=torch.int32, device=dev)
        lab = torch.zeros(n_sweeps, F, dtype=torch.int32, device=dev); best_lab = torch.zeros_like(lab)
        energy = []; best = 2 ** 64 - 1
        for sw in range(n_sweeps):
            for ph in range(n_phases):
                for a, b in zip(cuts, cuts[1:]): ops.sweep_phase(ph, a, b)
            ops.gather(G.LAB, idx, lab[sw])                      # before the bookkeeping: keeping a sweep flips the decode buffers
            e = ops.energy(G.LAB, 0, F)
            if device_step:
                ops.step(e)
                energy.append(int(e[0].item()) & (2 ** 64 - 1))
            else:
                energy.append(int(e[0].item()) & (2 ** 64 - 1))
                if energy[-1] < best:
                    best = energy[-1]; ops.keep_best()
            ops.gather(G.BEST_LAB, idx, best_lab[sw])
        torch.cuda.synchronize()
        return lab.cpu().numpy().view(np.uint32), best_lab.cpu().numpy().view(np.uint32), np.array(energy, np.uint64), n_phases
    finally:
        c.close()


def _first_difference(case, got, want, what):
    s, i = [int(x[0]) for x in np.nonzero(got != want)]
    cls = U.node_classes_numpy(case.col_ptr, case.adj_ptr, case.adj)
    return "%s differs from the oracle's trace first in sweep %d at node %d (class %d, K = %d, degree %d): label %d for %d; %d nodes differ in that sweep" % (
        what, s + 1, i, cls[i], case.col_ptr[i + 1] - case.col_ptr[i], case.adj_ptr[i + 1] - case.adj_ptr[i], got[s, i], want[s, i], int((got[s] != want[s]).sum()))


_trace_cache = {}


def _oracle_trace(name):
    if name not in _trace_cache:
        case = CASES[name]()
        _trace_cache[name] = O.view_selection_traced(_csr(case), case.adj_ptr, case.adj, O.default_mrf_params(max_sweeps=16, min_sweeps=16), n_sweeps=16)[2]
    return _trace_cache[name]


@pytest.mark.parametrize("pieces,device_step", [(1, True), (3, False)], ids=["whole-step", "three_ranges-keep_best"])
@pytest.mark.parametrize("name", ["tied1", "tied15", "boundary", "isolated"])
def test_every_sweep(name, pieces, device_step):
    """16 sweeps (four of them damped): the decoded labels and the best labeling after EVERY sweep, and every sweep's tracking energy,
    equal the oracle's trace -- a sweep that decodes wrongly without being the best one, or whose error the polish repairs, shows here.
    Cutting every phase into three node ranges changes nothing."""
    case = CASES[name]()
    tr = _oracle_trace(name)
    lab, best, energy, n_phases = _drive_sweeps(case, 16, pieces, device_step)
    assert n_phases == int(U.colouring_numpy(case.adj_ptr, case.adj).max()) + 1
    assert np.array_equal(lab, tr["lab"]), _first_difference(case, lab, tr["lab"], "the decode")
    assert np.array_equal(energy, tr["energy"]), (energy.tolist(), tr["energy"].tolist())
    assert np.array_equal(best, tr["best"]), _first_difference(case, best, tr["best"], "the best labeling")
    if name == "isolated":
        first = U.first_min_code_labels(case)
        assert np.all(lab == first[None, :]), _first_difference(case, lab, np.tile(first, (16, 1)), "the decode (numpy first argmin of the cost codes)")


def test_three_logical_shards_equal_the_single_solve():
    """tied costs over a part boundary: the ICM winner rule's (gain, id) order decides between nodes of different parts"""
    import torch
    import multigpu as G
    name = "tied1"
    case = CASES[name]()
    F = len(case.col_ptr) - 1
    lo, so = _oracle(name, "defaults")
    ctxs = [M.Context(0) for _ in range(3)]
    try:
        labels, (e, sweeps, icm), n_phases = G.logical_shards_view_selection(ctxs, _table(case), np.array(case.adj_ptr), np.array(case.adj), G.equal_parts(F, 3),
                                                                              M.viewsel.default_mrf_params(), torch.device("cuda:0"))
    finally:
        for c in ctxs: c.close()
    assert np.array_equal(labels, lo), "labels depend on the partition: %d differ" % int((labels != lo).sum())
    assert (e, sweeps, icm) == (so["energy_fixed"], so["sweeps"], so["icm_iters"])
