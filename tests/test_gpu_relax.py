"""rcp_relax (k_pdb_relax of librubiksearch.so) as a stage of its own: after every pop, merge AND relax every buffer of an AStarPlan
against the numpy restatement (tests/pattern_ref.py's Relaxed), in a built state -- "flood, lift, re-open", described there -- in
which nearly every candidate offers an OPEN node a lower g: nodes contested by several candidates, ties on g decided by c, winners
that are not the lowest c, offers from different strides of the workgroup's loop, a ragged last stride, weights whose product with g
rounds, a problem that ended in the same iteration, full pools.  Each point also asserts, on the restatement's counters, that the case
it exists for occurred (tests/test_pattern_host.py holds the same without a GPU).  All comparisons are exact.  GPU only."""
import pytest
import torch

from tests import pattern_ref as R
from tests.test_gpu_astar import DEV, Pair
from tests.test_gpu_search import scrambles

pytestmark = pytest.mark.gpu


def zero_scores(pair):
    pair.plan.beam.scores.zero_()


def end_one(pair):
    pair.ref.ended_by_hand = R.end_one(pair.ref)
    pair.plan.beam.active.copy_(torch.from_numpy(pair.ref.active).to(DEV))
    pair.compare("one problem ended by hand")


@pytest.mark.parametrize("case", R.scenario_cases(), ids=R.case_id)
def test_relax_stage_in_the_built_scenario(case):
    """A Pair with relax=True compares the whole state after pop, merge and relax, and holds that relax leaves flags, keys, scores
    and the persistent hash table byte for byte.  The doctoring is written to the restatement and copied to the device."""
    pair = Pair(case.cs, scrambles(case.cs, R.scenario_depths(case.P), seed=R.SEEDS[case.cs]), case.B, case.C, weight=case.weight,
                front="table", relax=True)
    plan, ref = pair.plan, pair.ref
    for _ in range(R.scenario_pre(case.cs, case.B)):
        pair.iterate(zero_scores)
    ref.overflowed = ref.overflow.copy()
    R.doctor(ref, case.jitter, case.mode)
    for name, dev in (("g", plan.g), ("state", plan.state), ("prio", plan.prio), ("score", plan.node_score)):
        dev.copy_(torch.from_numpy(getattr(ref, name)).to(DEV))
    pair.compare("doctored")
    pair.iterate(zero_scores, before_relax=end_one)
    ref.dropped, ref.duplicated = R.dropped_and_duplicated(ref, pair.new_masks)
    pair.iterate(zero_scores)
    print(R.case_id(case), ref.counters(), "dropped", ref.dropped, "duplicated", ref.duplicated)
    R.check_reached(case, ref)
