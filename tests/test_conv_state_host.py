"""The float64 reference of a stream whose taps change partway (stream_reference with a schedule) against an
independent source: the oracle's buffer-by-buffer float64 stream, which carries the input history itself and is simply
handed the new response.  test_conv_plan_state_gpu.py holds every conv route's set_ir to it."""
import numpy as np
import pytest

from test_conv_fdl_host import stream_reference


def _ir(T, L, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, L)) * np.exp(-np.arange(L) / (L / 4.0))).astype(np.float32).ravel()


# L = 1500: the history fills after 12 / 6 / 3 buffers; m switches before that and after it
@pytest.mark.parametrize("B,m", [(128, 5), (128, 15), (256, 2), (256, 9), (512, 1), (512, 6)])
def test_switched_reference_equals_the_oracle_stream(orc, B, m):
    T, L, n = 3, 1500, 20
    ir1, ir2 = _ir(T, L, 1), _ir(T, L, 2)
    rng = np.random.default_rng(B + m)
    xs = [rng.standard_normal(T * B).astype(np.float32) for _ in range(n)]
    refs = stream_reference(xs, [(0, ir1), (m, ir2)], T, B, L)
    assert len(refs) == n
    hist = np.zeros(T * L, np.float32)
    outs = [orc.conv_accel_stream(xs[i], ir1 if i < m else ir2, hist, L, B, T, f64=True) for i in range(n)]
    peak = max(np.abs(r).max() for r in refs)
    for i in range(n):
        assert np.abs(outs[i] - refs[i]).max() <= 1e-12 * peak, i
    # the switch is visible: the unswitched stream is far from it after m
    plain = stream_reference(xs, ir1, T, B, L)
    assert max(np.abs(plain[i] - refs[i]).max() for i in range(m)) <= 1e-12 * peak
    assert min(np.abs(plain[i] - refs[i]).max() for i in range(m, n)) > 1e-2 * peak


def test_schedule_with_one_entry_is_the_plain_reference():
    T, B, L = 2, 128, 700
    ir = _ir(T, L, 3)
    rng = np.random.default_rng(4)
    xs = [rng.standard_normal(T * B).astype(np.float32) for _ in range(9)]
    a, b = stream_reference(xs, ir, T, B, L), stream_reference(xs, [(0, ir)], T, B, L)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
