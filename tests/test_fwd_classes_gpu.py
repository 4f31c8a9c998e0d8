"""GPU suite (-m gpu): every forward-kernel width class, adjacent pair, folded launch and score-envelope edge of tests/fwd_cases.py on the
device, against the oracle byte for byte (status, consensus bytes, cell count; no capacity retry, no window may report an overflow).
Every case that the restated routing sends to k_fwd_dt also runs with VC_DT=0 (k_fwd on the same byte-packed rows): bytes, statuses,
cells, dp_rows and band_redo must agree, each form run twice -- a hazard between a row's store and the next row's pack shows as a
run-to-run difference.

The table covers what the seeded generator of test_gpu.py never produces: reads of exactly 64 * CPL columns, of 64 * CPL_prev + 1,
batches that straddle a class edge by one base, the 1 025 .. 2 048-column range (classes 20, 24, 32 and their pairs) that
test_randomised_sweep_fixed_seed's list of lengths skips, and score sets on the bounds of vc_row_packed, vc_dt_ok and vc_int16_ok.
Which instantiation ran is not observable: the routing asserted here is fwd_cases.route(), a restatement of the host's decisions,
evaluated with the row capacity the context really took (stats()["max_nodes"]).

Contexts are module-scoped and warm: the default-score contexts see the cases in table order -- classes 4 -> 64, the pairs, the folds --
and then class 8 again (test_class_8_again_on_the_warm_contexts), so every new batch shape re-plans workspaces that exist."""
import pytest

import fwd_cases as fc
from vechat_amd import capi
from vechat_amd.engine import HipContext

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def contexts(built):
    """(scores, max_nodes, overload, VC_DT) -> context, made on first use and kept for the module.  VC_DT is read in vc_create: it is set
    around the creation only."""
    made = {}
    recent = []          # the last two (scores, capacity) sets other than the default: the table keeps a set's cases together

    def get(case, mode, dt):
        key = (case.scores.key(), case.max_nodes, mode, dt)
        if case.scores is not fc.DEFAULT:
            if key[:2] in recent:
                recent.remove(key[:2])
            recent.append(key[:2])
            for old in recent[:-2]:
                for k in [k for k in made if k[:2] == old]:
                    made.pop(k).close()
            del recent[:-2]
        if key not in made:
            with pytest.MonkeyPatch.context() as mp:
                mp.setenv("VC_DT", dt)
                made[key] = HipContext(params=case.params(mode))
        return made[key]
    yield get
    for c in made.values():
        c.close()


FIRST = {}           # (case name, overload) -> what the first run of a case gave (test_class_8_again_on_the_warm_contexts)


def _run(ctx, case, mode, label):
    cons, status = ctx.consensus(case.batch(), retry_overflow=False)
    ref, pol, ost = fc.oracle(case, mode)
    st = ctx.stats()
    status = [int(x) for x in status]
    assert capi.VC_WIN_OVERFLOW not in status, (label, status, ctx.errinfo())
    assert status == [capi.VC_WIN_OK if p else capi.VC_WIN_UNPOLISHED for p in pol], (label, status, ctx.errinfo())
    for w in range(len(ref)):
        if cons[w] != ref[w]:
            at = next((i for i, (x, y) in enumerate(zip(cons[w], ref[w])) if x != y), min(len(cons[w]), len(ref[w])))
            raise AssertionError((label, "window", w, "first differing byte", at, len(cons[w]), len(ref[w])))
    assert st["cells"] == ost["cells"], (label, st["cells"], ost["cells"])
    return dict(cons=tuple(cons), status=status, cells=st["cells"], dp_rows=st["dp_rows"], band_redo=st["band_redo"]), st


def _check_case(contexts, case, mode):
    ctx = contexts(case, mode, "1")
    got, st = _run(ctx, case, mode, (case.name, mode, "VC_DT=1"))
    # the routing, judged with the capacity the context really took (grow-only on a warm context)
    inst, form, wide = case.route(NC=st["max_nodes"])
    assert (inst, form) == (case.inst, case.form), (case.name, st["max_nodes"], inst, form, wide)
    if case.max_nodes:
        assert st["max_nodes"] == case.nc()
    if form == "dt":
        seen = [got, _run(ctx, case, mode, (case.name, mode, "VC_DT=1, again"))[0]]
        c0 = contexts(case, mode, "0")
        for rep in range(2):
            g0, st0 = _run(c0, case, mode, (case.name, mode, "VC_DT=0", rep))
            assert case.route(NC=st0["max_nodes"], vc_dt=False)[1] == "packed"
            seen.append(g0)
        assert all(x == seen[0] for x in seen[1:]), (case.name, mode, [(x["cells"], x["dp_rows"], x["band_redo"], x["status"]) for x in seen])
    FIRST.setdefault((case.name, mode), got)
    return got


@pytest.mark.parametrize("mode", [0, 1], ids=["hap", "linear"])
@pytest.mark.parametrize("case", fc.CASES, ids=repr)
def test_case_against_the_oracle(contexts, case, mode):
    _check_case(contexts, case, mode)


def test_the_dt_bound_splits_the_two_capacities(contexts):
    """vc_dt_ok is judged with the workspaces' row capacity: the two contexts took 3 392 and 3 456 rows, one on each side of
    4 * 513 + (NC + 521) * 16 <= 65 000, and the window's graph (fwd_cases.DT_ROWS rows at the end of the build) fills the smaller one to 99 %."""
    caps = []
    for nc in fc.DT_NC:
        case = fc.BY_NAME[f"Ddt_nc{nc}"]
        ctx = contexts(case, 0, "1")
        _run(ctx, case, 0, (case.name, "capacity"))
        caps.append(ctx.stats()["max_nodes"])
    print("vc_dt_ok capacities taken:", caps)
    assert tuple(caps) == fc.DT_NC
    assert fc.dt_ok(4, -6, -16, caps[0], 8) and not fc.dt_ok(4, -6, -16, caps[1], 8)
    assert 0.9 * caps[0] <= fc.DT_ROWS <= caps[0]


@pytest.mark.parametrize("mode", [0, 1], ids=["hap", "linear"])
def test_class_8_again_on_the_warm_contexts(contexts, mode):
    """after classes 4 -> 64, the pairs and the folds, the same contexts take class 8 again: workspaces sized for 64 columns per lane and
    the largest capacity so far are re-planned for the narrow batch, and the result equals the first one"""
    wide, narrow = fc.BY_NAME["A64"], fc.BY_NAME["A8"]
    if (narrow.name, mode) not in FIRST:                 # (run on its own: the same order in short)
        _check_case(contexts, narrow, mode)
    first = FIRST[(narrow.name, mode)]
    _check_case(contexts, wide, mode)
    nc_warm = contexts(narrow, mode, "1").stats()["max_nodes"]
    again = _check_case(contexts, narrow, mode)
    assert again == first
    assert contexts(narrow, mode, "1").stats()["max_nodes"] >= nc_warm >= narrow.nc()          # capacities are grow-only
