"""The seeded walks of tests/walks.py replayed on the device: every row of WALKS by per-buffer calls, batched at the
tape's cuts, and batched with every block 4 bytes off 16-byte alignment; where the header allows d_out == d_in (delay,
dynamics, gate, limiter, and reverb with one output) once more in place.  Every buffer's outputs are the host twin's under
differing(), and at every check marker (behind every set, refused set and reset, and at the end) the carried state the
plan exposes is the host actor's recorded state under same(): bits, no tolerance.  A refused set raises GabError
naming the value the host rule names, and the next check finds tables and a pending ramp unchanged.  The spectrum
plan's transform is no bit twin: its frame counts, history, window and position are exact, and the rows of every frame
are the bits of a single-frame plan given the raw samples the host holds for that frame (test_edges_gpu.DevSpec); on
the complex walk they are also within test_spectrum_gpu's bound of the float64 transform.  That the walks
reach what they are for, and would catch a defective twin, is shown on the host (tests/test_walks_host.py)."""
import pytest

import numpy as np

import conv_pair_twin as tw
import spectrum_twin as st
from plan_helpers import gab  # noqa: F401 (the fixture)
from test_edges_gpu import DEVS
from test_edges_host import differing, play
from walks import WALKS, walk, walk_id, window_kind

pytestmark = pytest.mark.gpu

IN_PLACE = [w for w in WALKS if w.plan in ("delay", "dyn", "gate", "lim") or (w.plan == "reverb" and w.shape[3] == 1)]


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
    return actor


@pytest.mark.parametrize("how", ["per-buffer", "batched", "batched-offset"])
@pytest.mark.parametrize("w", WALKS, ids=walk_id)
def test_the_plan_is_its_twin_along_the_walk(gab, w, how):
    replay(gab, w, batch=how != "per-buffer", offset=how == "batched-offset")


@pytest.mark.parametrize("w", IN_PLACE, ids=walk_id)
def test_the_plan_is_its_twin_along_the_walk_in_place(gab, w):
    replay(gab, w, batch=False, inplace=True)


@pytest.mark.parametrize("w", [w for w in WALKS if w.plan == "spec" and w.shape[3] == "complex"], ids=walk_id)
def test_the_walked_complex_frames_are_within_the_bound_of_the_float64_transform(gab, w):
    """test_spectrum_gpu's bound, FACTOR c_twin capped at 1e-5, on every frame of the walk: a transform wrong on the
    walked plan and on the single-frame plan alike would pass the comparison of their bits.  c_twin is the twin's
    figure on the same frames; a frame whose pair is all zeros (a one-hot window on a zero of the history) has no level
    and must be zeros.  Measured (profiles/r23_walks_three_plans.txt): c_gpu / c_twin 3.99 over the walk; at most 1.98
    on its Hann frames, 1.50 under the seeded positive window, 3.99 on its two one-hot frames, which
    tests/test_spectrum_gpu.py holds to KNOWN_FACTOR = 7.3 and this test to the 4 of every other frame."""
    from test_spectrum_gpu import FACTOR, cplx
    seen = replay(gab, w, batch=False).seen
    frames = np.stack([win[None, :] * raw for raw, win, _ in seen])
    assert frames.dtype == np.float32 and len(frames) >= 16
    X, X64 = cplx(np.stack([rows for _, _, rows in seen])), st.truth(frames)
    c, level = st.figures(st.spectra(frames), X64)
    cg, _ = st.figures(X, X64)
    live = level > 0
    c_twin = tw.c_max(c)
    print("\nspectrum walk %s: %d frames, %d of %d live, c_twin %.3g c_gpu %.3g ratio %.2f"
          % (walk_id(w), len(frames), live.sum(), live.size, c_twin, np.nanmax(cg), np.nanmax(cg) / c_twin))
    kinds = np.array([window_kind(win) for _, win, _ in seen])
    for kind in sorted(set(kinds)):
        print("    %s windows: %d frames, c_gpu / c_twin at most %.2f"
              % (kind, (kinds == kind).sum(), np.nanmax(cg[kinds == kind]) / c_twin))
    assert 0 < c_twin <= 1e-6 and live.mean() > 0.5 and not X[~live].any()
    assert (cg[live] <= min(FACTOR * c_twin, 1e-5)).all(), np.nanmax(cg) / c_twin
