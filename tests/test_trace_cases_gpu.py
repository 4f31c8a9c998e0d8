"""GPU suite (-m gpu): the case table of tests/trace_cases.py on the device -- hand-built chain-plus-skip windows that put a path on the
last lane of the stored band and one column beyond it, in-edges at the distance and in-degree bounds of k_tracew and the row records,
read-backs on both sides of the kept ring, jumps below the sliding table window and 15 .. 33 tied sinks.

Every case: consensus bytes and status equal to the oracle in both overloads, under both forward forms (VC_DT unset / VC_DT=0) and twice
per form on warm module-scoped contexts; bytes and counters identical across the four runs.  Linear overload: trace_steps equals the
summed lengths of the oracle's pair lists; cases marked exact: band_redo == number of alignments classified `outside` by the restated band
(the others are `clear`: they cannot be redone); haplotype overload: band_redo >= that number (the re-alignment rounds add their own).
Nothing asserted here is copied from a device run: the numbers come from trace_cases.py's restatement and the oracle."""
import pytest

import fwd_cases as fc
import trace_cases as tc
from vechat_amd import capi
from vechat_amd.engine import HipContext

pytestmark = pytest.mark.gpu
COUNTERS = ("cells", "dp_rows", "band_redo", "far_row_reads", "trace_steps", "trace_spec", "trace_rounds")


@pytest.fixture(scope="module")
def contexts(built):
    """(overload, VC_DT, VC_RESOLVE_FORCE_DFS) -> context, made on first use and kept for the module; both switches are read in vc_create"""
    made = {}

    def get(case, mode, dt, dfs=False):
        key = (mode, dt, dfs)
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("VC_DT", dt)
                if dfs:
                    mp.setenv("VC_RESOLVE_FORCE_DFS", "1")
                else:
                    mp.delenv("VC_RESOLVE_FORCE_DFS", raising=False)
                made[key] = HipContext(params=case.params(mode))
        return made[key]
    yield get
    for c in made.values():
        c.close()


def _run(ctx, case, mode, label):
    cons, status = ctx.consensus(case.batch(), retry_overflow=False)
    ref, pol, ost = fc.oracle(case, mode)
    st = ctx.stats()
    status = [int(x) for x in status]
    assert status == [capi.VC_WIN_OK if p else capi.VC_WIN_UNPOLISHED for p in pol], (label, status, ctx.errinfo())
    for w in range(len(ref)):
        if cons[w] != ref[w]:
            at = next((i for i, (x, y) in enumerate(zip(cons[w], ref[w])) if x != y), min(len(cons[w]), len(ref[w])))
            raise AssertionError((label, "window", w, case.wins()[w].tag, "first differing byte", at, len(cons[w]), len(ref[w])))
    assert st["cells"] == ost["cells"], (label, st["cells"], ost["cells"])
    return dict(cons=tuple(cons), status=status, **{k: st[k] for k in COUNTERS})


def _four_runs(contexts, case, mode, dfs=False):
    seen = []
    for dt in ("1", "0") if case.banded() else ("1",):
        ctx = contexts(case, mode, dt, dfs)
        for rep in range(2):
            seen.append(_run(ctx, case, mode, (case.name, mode, "VC_DT=" + dt, rep)))
    print(case.name, "mode", mode, {k: seen[0][k] for k in COUNTERS}, "outside", case.outside(), [w.tag for w in case.wins()])
    assert all(x == seen[0] for x in seen[1:]), (case.name, mode, [{k: x[k] for k in COUNTERS} for x in seen])
    return seen[0]


@pytest.mark.parametrize("mode", [0, 1], ids=["hap", "linear"])
@pytest.mark.parametrize("case", [c for c in tc.CASES if c.name[0] != "T"], ids=repr)
def test_case_against_the_oracle_and_the_restated_band(contexts, case, mode):
    got = _four_runs(contexts, case, mode)
    if mode == 1:
        assert got["trace_steps"] == tc.oracle_steps(case), (case, got["trace_steps"], tc.oracle_steps(case))
        if case.exact:
            assert got["band_redo"] == case.outside(), (case, got["band_redo"], case.outside(), case.klasses())
        if case.far is not None:
            assert (got["far_row_reads"] > 0) == case.far and (case.far or got["far_row_reads"] == 0), (case, got["far_row_reads"])
        if case.chain:
            # per alignment: L steps, all of them speculated, ceil(L / 8) rounds (trace_cases.chain_walk); two alignments per window
            want = [sum(2 * tc.chain_walk(w.L)[i] for w in case.wins()) for i in range(3)]
            assert [got["trace_steps"], got["trace_spec"], got["trace_rounds"]] == want, (got, want)
    else:
        assert got["band_redo"] >= case.outside(), (case, got["band_redo"], case.outside())


@pytest.mark.parametrize("dfs", [False, True], ids=["closure", "force_dfs"])
@pytest.mark.parametrize("mode", [0, 1], ids=["hap", "linear"])
@pytest.mark.parametrize("case", [c for c in tc.CASES if c.name[0] == "T"], ids=repr)
def test_tied_sinks(contexts, case, mode, dfs):
    """15 / 16 / 17 / 33 sinks tied at the end cell (the tie memory holds VC_MAXTIE = 16, tie_over the rest); the order of the sinks is not
    unique, so bytes, status and (linear overload) the number of moves only"""
    got = _four_runs(contexts, case, mode, dfs)
    if mode == 1:
        assert got["trace_steps"] == tc.oracle_steps(case)
