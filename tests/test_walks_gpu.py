"""The seeded walks of tests/walks.py replayed on the device: every row of WALKS by per-buffer calls, batched at the
tape's cuts, and batched with every block 4 bytes off 16-byte alignment; where the header allows d_out == d_in (delay,
dynamics, gate, and reverb with one output) once more in place.  Every buffer's outputs are the host twin's under
differing(), and at every check marker (behind every set, refused set and reset, and at the end) the carried state the
plan exposes is the host actor's recorded state under same(): bits, no tolerance.  A refused set raises GabError
naming the value the host rule names, and the next check finds tables and a pending ramp unchanged.  That the walks
reach what they are for, and would catch a defective twin, is shown on the host (tests/test_walks_host.py)."""
import pytest

from plan_helpers import gab  # noqa: F401 (the fixture)
from test_edges_gpu import DEVS
from test_edges_host import differing, play
from walks import WALKS, walk, walk_id

pytestmark = pytest.mark.gpu

IN_PLACE = [w for w in WALKS if w.plan in ("delay", "dyn", "gate") or (w.plan == "reverb" and w.shape[3] == 1)]


def replay(gab, w, batch, offset=False, inplace=False):
    ops, want, _, _ = walk(*w)
    actor = DEVS[w.plan](gab, offset, *w.shape)
    actor.inplace = inplace
    try:
        got = play(ops, actor, batch=batch)                          # the state is compared at every check on the way
        assert actor.checked == sum(op[0] == "check" for op in ops)
        assert differing(got, want) == []
    finally:
        actor.close()


@pytest.mark.parametrize("how", ["per-buffer", "batched", "batched-offset"])
@pytest.mark.parametrize("w", WALKS, ids=walk_id)
def test_the_plan_is_its_twin_along_the_walk(gab, w, how):
    replay(gab, w, batch=how != "per-buffer", offset=how == "batched-offset")


@pytest.mark.parametrize("w", IN_PLACE, ids=walk_id)
def test_the_plan_is_its_twin_along_the_walk_in_place(gab, w):
    replay(gab, w, batch=False, inplace=True)
