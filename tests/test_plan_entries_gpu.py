"""What the entry points of the eleven track plans answer before they launch anything, through the raw C functions.

One table: for every plan a create with tracks = 0, a create with the plan's own first refused argument, a process
with a null input, a process_batch with n_buffers = 0, the params / gains call with a null out-pointer (where the
plan has one), reset(NULL) and destroy(NULL) -- each with its return code and the whole gab_last_error() text, written
out here because a caller may match on it.  Every one of them returns on the host.  The plan that heard all of this
then processes one buffer of a ramp and gives the bits of a fresh plan.  Shapes: the smallest that create every plan.

A row may end in a dict of what its plan has beside the common form: `unset`, the text with which process and
process_batch answer on a plan that no set has reached yet (the crossover), and `prepare`, the set that comes before
the final buffer, on both plans; `also_null`, out-pointers of process beside input and output that the entry lists as
needed (the spectrum plan's n_frames); `final_bufsize`, the bufsize of the two plans of the final comparison where a
buffer of B = 8 writes nothing (the spectrum plan at hop 32 emits its first frame with sample 32: B = 32 is the smaller
of the two shapes that do, the other being bufsize = hop = 1024).
"""
import ctypes as C

import numpy as np
import pytest

from plan_helpers import bits, dev, gab, host  # noqa: F401 (gab: the fixture)

pytestmark = pytest.mark.gpu

T, B = 3, 8
INVALID, UNSUPPORTED = -1, -3


def xover_splits(gab, lib, h, stream):
    rows = dev(np.tile(gab.crossover_rows(1000.0), (T, 1, 1)))
    assert lib.gab_xover_set_splits(h, C.c_void_p(rows.data_ptr()), stream) == 0


# name: (the create arguments behind (tracks, bufsize), [(refused create arguments from tracks on, code, text)],
#        the arguments of process_batch between input and stream (process: without n), floats of one buffer's output,
#        the call that exposes the ramped table or None, what a null plan is called[, the dict of the docstring])
PLANS = {
    "eq": ((1,), [((T, B, 0), INVALID, "sections must be 1..16")], "out n", T * B, None, "null plan"),
    "mix": ((1,), [((T, B, 0), INVALID, "buses must be 1..64")], "out n layout", B, "gab_mix_gains", "null pointer"),
    "delay": ((4, 0), [((T, B, 4, 2), INVALID, "interp must be GAB_DELAY_LINEAR or GAB_DELAY_LAGRANGE3")],
              "out n", T * B, "gab_delay_params", "null pointer"),
    "meter": ((1,), [((T, B, 0), INVALID, "window must be 1..64")], "out n", T * 8, None, "null pointer"),
    "resample": ((2, 1, 4), [((T, (1 << 20) + 1, 2, 1, 4), INVALID, "bufsize must be <= 2^20"),
                             ((T, B, 1023, 1, 256), UNSUPPORTED,
                              "a table of up * taps = 261888 floats (up reduced) is more than 16384")],
                 "out n counts", T * 2 * B, None, "null pointer"),
    "dyn": ((1,), [((T, B, 3), INVALID, "link must be a power of two in 1..64")],
            "key out extra n", T * B, "gab_dyn_params", "null pointer"),
    "reverb": ((4, 1, 64), [((T, B, 5, 1, 64), INVALID, "lines must be 4, 8 or 16")],
               "out n", T * B, "gab_reverb_params", "null pointer"),
    "gate": ((1,), [((T, B, 3), INVALID, "link must be a power of two in 1..64")],
             "key out extra n", T * B, "gab_gate_params", "null pointer"),
    "xover": ((2,), [((T, B, 5), INVALID, "bands must be 2..4")], "out n", 2 * T * B, None, "null pointer",
              {"unset": "no splits have been set: gab_xover_set_splits comes first", "prepare": xover_splits}),
    "lim": ((5, 1), [((T, B, 9, 1), INVALID, "lookahead_log2 must be 2..8"),
                     ((T, B, 5, 3), INVALID, "link must be a power of two in 1..64"),
                     ((T, B, 5, 2), INVALID, "tracks must be a multiple of link")],
            "out extra n", T * B, "gab_lim_params", "null pointer"),
    "spec": ((32, 1, 0), [((T, B, 16, 1, 0), INVALID, "hop must be 32..1024"),
                          ((T, B, 32, 2, 0), INVALID, "mode must be GAB_SPEC_COMPLEX or GAB_SPEC_POWER"),
                          ((T, B, 32, 1, 65), INVALID, "bands must be 0..64"),
                          ((T, B, 32, 0, 4), INVALID, "bands need GAB_SPEC_POWER (complex rows have no band form)")],
             "out n frames", T * 513, None, "null pointer", {"also_null": ("frames",), "final_bufsize": 32}),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_entries(gab, name):
    lib, stream = gab._capi.lib, gab.ops._stream
    rest, refused_creates, form, out_floats, expose, null_plan = PLANS[name][:6]
    more = PLANS[name][6] if len(PLANS[name]) > 6 else {}
    fn = lambda what: getattr(lib, "gab_%s_%s" % (name, what))       # noqa: E731

    def answers(rc, code, text):
        assert rc == code
        assert lib.gab_last_error().decode() == text

    def create(*args):
        h = C.c_void_p(0xdead)                  # (a refusal leaves null behind, not what was there)
        return fn("create")(C.byref(h), *args), h

    def process_args(h, x, out, n=None, null=()):
        counts, frames = (C.c_int * 1)(), C.c_int(0)
        a = {"key": None, "out": out, "extra": None, "layout": 0, "counts": counts, "n": n, "frames": C.byref(frames)}
        a.update({k: None for k in null})
        return [h, x] + [a[k] for k in form.split() if k != "n" or n is not None] + [stream()]

    def one_buffer(h, B):
        x = dev(np.arange(T * B, dtype=np.float32) / 16.0 - 0.5)
        out = dev(np.full(out_floats, np.nan, np.float32))
        assert fn("process")(*process_args(h, C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()))) == 0
        return bits(host(out))

    who = "gab_%s_create: " % name
    rc, h = create(0, B, *rest)
    answers(rc, INVALID, who + "tracks and bufsize must be > 0")
    assert h.value is None
    for args, code, text in refused_creates:
        rc, h = create(*args)
        answers(rc, code, who + text)
        assert h.value is None
    answers(fn("create")(None, T, B, *rest), INVALID, who + "null plan pointer")

    rc, h = create(T, B, *rest)
    assert rc == 0 and h.value
    out = dev(np.zeros(out_floats, np.float32))
    x = dev(np.zeros(T * B, np.float32))
    px, po = C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr())
    answers(fn("process")(*process_args(h, None, po)), INVALID, "gab_%s_process: null pointer" % name)
    answers(fn("process_batch")(*process_args(h, None, po, 1)), INVALID, "gab_%s_process_batch: null pointer" % name)
    answers(fn("process_batch")(*process_args(h, px, po, 0)), INVALID,
            "gab_%s_process_batch: n_buffers must be > 0" % name)
    answers(fn("process_batch")(*process_args(h, None, po, 0)), INVALID,    # null is looked at before n_buffers
            "gab_%s_process_batch: null pointer" % name)
    for k in more.get("also_null", ()):
        answers(fn("process")(*process_args(h, px, po, null=(k,))), INVALID, "gab_%s_process: null pointer" % name)
        answers(fn("process_batch")(*process_args(h, px, po, 1, null=(k,))), INVALID,
                "gab_%s_process_batch: null pointer" % name)
    if "unset" in more:
        answers(fn("process")(*process_args(h, px, po)), INVALID, "gab_%s_process: %s" % (name, more["unset"]))
        answers(fn("process_batch")(*process_args(h, px, po, 1)), INVALID,
                "gab_%s_process_batch: %s" % (name, more["unset"]))
    if expose:
        b, n = C.c_void_p(), C.c_size_t(0)
        answers(getattr(lib, expose)(h, None, C.byref(b), C.byref(n)), INVALID, expose + ": null pointer")
    answers(fn("reset")(None, stream()), INVALID, "gab_%s_reset: %s" % (name, null_plan))
    answers(fn("destroy")(None), INVALID, "gab_%s_destroy: %s" % (name, null_plan))

    Bf = more.get("final_bufsize", B)
    if Bf != B:                                  # the plan that heard all of the above has its twin at the final bufsize
        assert fn("destroy")(h) == 0
        rc, h = create(T, Bf, *rest)
        assert rc == 0
        x = dev(np.zeros(T * Bf, np.float32))
        answers(fn("process")(*process_args(h, None, po)), INVALID, "gab_%s_process: null pointer" % name)
        answers(fn("process_batch")(*process_args(h, C.c_void_p(x.data_ptr()), po, 0)), INVALID,
                "gab_%s_process_batch: n_buffers must be > 0" % name)
    rc, fresh = create(T, Bf, *rest)
    assert rc == 0
    for plan in (h, fresh):
        if "prepare" in more:
            more["prepare"](gab, lib, plan, stream())
    got, want = one_buffer(h, Bf), one_buffer(fresh, Bf)
    assert np.array_equal(got, want)
    assert not np.array_equal(want, bits(np.full(out_floats, np.nan, np.float32)))   # (the buffer was written)
    assert fn("destroy")(h) == 0 and fn("destroy")(fresh) == 0
