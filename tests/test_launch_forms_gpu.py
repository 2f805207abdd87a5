"""Every launch form of the three host dispatchers that pick a kernel from the shape, held to the oracle.

gab_fdtd_process / launch_step, gab_dwg and gab_modal_bank choose a kernel or a template instantiation from the shape.
Each has a form query (gab_debug_fdtd_form, gab_debug_dwg_route, gab_debug_modal_launch) that runs the same host
function as the launcher.  A case here first asserts that the query names the form the case is listed under, then holds
the device to the oracle as test_gpu_parity.py does: bit for bit for the FDTD and the waveguides, the project's 1e-5 of
the float64-accumulated peak for the modal sums, and bit for bit for one mode alone.  The last test builds the census of
forms from the parametrisation lists below and fails when a form of a query has no case.

Shapes are the smallest that take the form: the thresholds are written beside each list.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gab():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    import gpuaudiobench_amd as g
    return g


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a).ravel(), bits(b).ravel())


# =====================================================================================================================
# FDTD
# =====================================================================================================================
T_FDTD, B_FDTD = 3, 12
CALLS = ((0, 1), (1, 6), (7, 5))            # odd, even, odd: the ping-pong pair ends a call either way round


def fdtd_params(gab, orc, dims, steps=3, src=None, rcv=None):
    """The oracle's parameters for a room and the library's, field for field the same (rooms with a side of 3 and
    hand-set cells are not gab_fdtd_default_params')."""
    P = orc.fdtd_params(*dims)
    P.steps_per_sample = steps
    if src is not None:
        P.src_x, P.src_y, P.src_z = src
    if rcv is not None:
        P.rcv_x, P.rcv_y, P.rcv_z = rcv
    G = gab._capi.FdtdParams(P.nx, P.ny, P.nz, P.src_x, P.src_y, P.src_z, P.rcv_x, P.rcv_y, P.rcv_z,
                             P.steps_per_sample, P.dt_over_rho_dx, P.rho_c2_dt_over_dx, P.absorption)
    return P, G


def run_fdtd_rounds(gab, orc, plan, P, form, seeds=(7, 8), expect_output=False):
    """Three calls on one plan, output and field against the oracle after each; a reset; the same with another seed."""
    import torch
    T, B = T_FDTD, B_FDTD
    for seed in seeds:
        x = orc.Rand(seed).bipolar(T * B)
        xd = dev(x)
        grids = orc.fdtd_grids(P)
        ref = np.zeros(T * B, np.float32)
        out = torch.zeros(T * B, device="cuda")
        for first, cnt in CALLS:
            assert plan.form(T, cnt)[0] == form, (first, cnt)
            orc.fdtd(P, grids, x, ref, T, B, first, cnt, fused=True)
            plan.process(xd, out, T, B, first, cnt)
            assert same(host(out), ref), (seed, first, cnt)
            assert same(host(plan.pressure()), grids[0]), (seed, first, cnt)
        assert np.abs(grids[0]).max() > 0
        if expect_output:
            assert np.count_nonzero(ref) >= 3 * T
        plan.reset()
        assert not host(plan.pressure()).any()


# form -> rooms (nx, ny, nz), steps_per_sample, "auto" | "step"
#   sample_tile   every side <= 56 and three steps per sample; tiles of 4 x 4 in (y, z), halo of 3
#   lds_*         nx % 4 == 0 and 16 < nx / 4 <= 64: 32 lanes up to nx = 128, 64 above; the taller tile from
#                 ceil(ny / (512 / lanes)) * nz >= 1024 workgroups on
#   step_vec4     every other nx % 4 == 0;   step_scalar   nx % 4 != 0  (block widths 16, 32, 64 by nx)
FDTD_ROOMS = {
    "resident": [((20, 20, 20), 3, "auto")],
    "sample_tile": [((5, 4, 4), 3, "step"), ((7, 9, 11), 3, "step"), ((20, 20, 20), 3, "step"), ((33, 7, 9), 3, "step"),
                    ((56, 56, 56), 3, "step"), ((56, 3, 5), 3, "step"), ((13, 56, 6), 3, "step")],
    "lds_32x8": [((72, 20, 9), 3, "step"), ((128, 5, 7), 3, "step"), ((68, 9, 3), 3, "step")],
    "lds_32x16": [((68, 17, 512), 3, "step")],                  # two tile rows, the second of one row; 2 * 512 = 1024
    "lds_64x4": [((132, 9, 7), 3, "step"), ((256, 4, 5), 3, "step")],
    "lds_64x8": [((256, 8, 1024), 3, "step")],
    "step_vec4": [((60, 9, 7), 3, "step"), ((64, 5, 70), 3, "step"), ((260, 6, 5), 3, "step"),
                  ((20, 57, 20), 3, "step"), ((20, 20, 57), 3, "step"),          # one side past the tile form's 56
                  ((20, 20, 20), 1, "step"), ((20, 20, 20), 2, "step"), ((20, 20, 20), 4, "step")],
    "step_scalar": [((57, 9, 7), 3, "step"), ((130, 6, 5), 3, "step"), ((301, 5, 4), 3, "step"), ((33, 7, 9), 2, "step"),
                    ((7, 9, 11), 2, "step"), ((57, 20, 20), 3, "step")],
}
FDTD_CASES = [(form, dims, steps, mode) for form, rooms in FDTD_ROOMS.items() for dims, steps, mode in rooms]


@pytest.mark.parametrize("form,dims,steps,mode", FDTD_CASES,
                         ids=["%s-%dx%dx%d-s%d" % (f, d[0], d[1], d[2], s) for f, d, s, m in FDTD_CASES])
def test_fdtd_form(gab, orc, form, dims, steps, mode):
    """A room per kernel form of gab_fdtd_process, with the fused source add and receiver tap of the call path (not
    gab_fdtd_step's null arguments): outputs and the pressure field bit for bit the oracle's over three calls, twice."""
    P, G = fdtd_params(gab, orc, dims, steps)
    plan = gab.FdtdPlan(G)
    plan.set_form(mode)
    assert plan.resident()[0] == (form == "resident")
    run_fdtd_rounds(gab, orc, plan, P, form)
    plan.close()


# (source, receiver) in a 20^3 room cut into 4 x 4 tiles: a tile's first corner and another's last corner; one cell for
# both; the source in the first cell inside the damped shell
TILE_CELLS = {
    "corners": ((9, 8, 8), (12, 11, 11)),
    "same_cell": ((10, 9, 10), (10, 9, 10)),
    "beside_shell": ((1, 1, 1), (3, 2, 2)),
}


@pytest.mark.parametrize("which", list(TILE_CELLS))
def test_fdtd_sample_tile_source_and_receiver_on_tile_edges(gab, orc, which):
    """The tile kernel's guarded receiver store and source add, where the owning thread is on a tile's edge."""
    src, rcv = TILE_CELLS[which]
    if which == "corners":
        assert src[1] % 4 == 0 and src[2] % 4 == 0 and rcv[1] % 4 == 3 and rcv[2] % 4 == 3
    P, G = fdtd_params(gab, orc, (20, 20, 20), 3, src, rcv)
    plan = gab.FdtdPlan(G)
    plan.set_form("step")
    run_fdtd_rounds(gab, orc, plan, P, "sample_tile", expect_output=True)
    plan.close()


def test_fdtd_graph_cache_hits_and_evictions(gab, orc):
    """The plan's own graph cache (calls of 24 launches and more): the key is (in, out, tracks, bufsize, first, n, the
    current pressure array).  (0, 8) four times on the same tensors keeps the key (24 swaps): calls two and four are
    hits.  Five further keys in a row evict from the four entries; then the first key again, twice.  The oracle makes
    the same calls; outputs and field after every one."""
    import torch
    T, B = 3, 8
    P, G = fdtd_params(gab, orc, (72, 20, 9))
    plan = gab.FdtdPlan(G)
    plan.set_form("step")
    x = orc.Rand(5).bipolar(T * B)
    xd = dev(x)
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    out = torch.zeros(T * B, device="cuda")
    assert plan.form(T, 3) == ("lds_32x8", False)               # 3 + 9 launches: enqueued one by one
    assert plan.form(T, 7) == ("lds_32x8", True)                # 3 + 21
    assert plan.form(T, 8, capturing=True) == ("lds_32x8", False)
    # (first, n): n = 7 swaps the pair an odd number of times, so the calls behind it have the other array in their key
    calls = [(0, 8)] * 4 + [(0, 7), (0, 8), (1, 7), (1, 7), (0, 7)] + [(0, 8), (0, 8)]
    keys, current = [], 0
    for first, cnt in calls:
        keys.append((first, cnt, current))
        current ^= (cnt * 3) & 1
    assert len(set(keys[4:9])) == 5 and keys[0] not in keys[4:9] and keys[9] == keys[0]
    for k, (first, cnt) in enumerate(calls):
        assert plan.form(T, cnt)[1] is True
        orc.fdtd(P, grids, x, ref, T, B, first, cnt, fused=True)
        plan.process(xd, out, T, B, first, cnt)
        assert same(host(out), ref), k
        assert same(host(plan.pressure()), grids[0]), k
    assert np.abs(grids[0]).max() > 0
    orc.fdtd(P, grids, x, ref, T, B, 2, 3, fused=True)           # and a call beside the cache
    plan.process(xd, out, T, B, 2, 3)
    assert same(host(out), ref) and same(host(plan.pressure()), grids[0])
    plan.close()


def capture_on_side_stream(record):
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            record()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return graph


# room -> (form outside a capture, form inside)
CAPTURE_ROOMS = {(20, 20, 20): ("resident", "sample_tile"), (72, 20, 9): ("resident", "lds_32x8")}


@pytest.mark.parametrize("dims", list(CAPTURE_ROOMS))
def test_fdtd_process_inside_a_callers_capture(gab, orc, dims):
    """gab_fdtd_process recorded into a caller's graph takes the step kernels; a whole buffer of 12 samples swaps the
    ping-pong pair an even number of times, so replay k is call k + 1 on the fields (one plain call came first: the
    strips exist).  The captured call itself moved nothing."""
    import torch
    T, B = T_FDTD, B_FDTD
    outside, inside = CAPTURE_ROOMS[dims]
    P, G = fdtd_params(gab, orc, dims)
    plan = gab.FdtdPlan(G)
    assert plan.form(T, B)[0] == outside and plan.form(T, B, capturing=True) == (inside, False)
    x = orc.Rand(3).bipolar(T * B)
    xd = dev(x)
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    out = torch.zeros(T * B, device="cuda")
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    plan.process(xd, out, T, B, 0, B)
    torch.cuda.synchronize()
    assert same(host(out), ref) and same(host(plan.pressure()), grids[0])
    graph = capture_on_side_stream(lambda: plan.process(xd, out, T, B, 0, B))
    assert same(host(out), ref) and same(host(plan.pressure()), grids[0])       # recorded, not run
    for k in range(3):
        graph.replay()
        orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
        torch.cuda.synchronize()
        assert same(host(out), ref), k
        assert same(host(plan.pressure()), grids[0]), k
    assert np.count_nonzero(ref) >= 3 * T
    # a plain call behind the replays goes on from their fields
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    plan.process(xd, out, T, B, 0, B)
    assert same(host(out), ref) and same(host(plan.pressure()), grids[0])
    del graph
    plan.close()


@pytest.mark.parametrize("dims", list(CAPTURE_ROOMS))
def test_fdtd_captured_calls_that_are_refused_leave_plan_and_capture_alone(gab, orc, dims):
    """The rule of "Captured calls" (include/gab_c_api.h): a captured call that would swap the ping-pong pair an odd
    number of times, or that would have to grow the strips, is refused by its text before anything is touched; the
    capture goes on, and the even call recorded behind the refusals replays as successive calls."""
    import torch
    T, B = T_FDTD, B_FDTD
    P, G = fdtd_params(gab, orc, dims)
    plan, fresh = gab.FdtdPlan(G), gab.FdtdPlan(G)
    x = orc.Rand(4).bipolar(T * B)
    xd = dev(x)
    x2, out2 = torch.zeros(T * 2 * B, device="cuda"), torch.zeros(T * 2 * B, device="cuda")
    grids = orc.fdtd_grids(P)
    ref = np.zeros(T * B, np.float32)
    out = torch.zeros(T * B, device="cuda")
    orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
    plan.process(xd, out, T, B, 0, B)
    torch.cuda.synchronize()
    was = plan.form(T, B), plan.form(T, 1)

    def record():
        with pytest.raises(gab.GabError, match="even number of times") as e:
            plan.process(xd, out, T, B, 0, 1)                      # 1 or 3 swaps
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
        with pytest.raises(gab.GabError, match="strips cannot grow") as e:
            plan.process(x2, out2, T, 2 * B, 0, 2 * B)              # even, but twice the strips
        assert e.value.code == gab._capi.GAB_ERR_INVALID_ARG
        with pytest.raises(gab.GabError, match="strips cannot grow"):
            fresh.process(xd, out, T, B, 0, B)                     # a plan's first call
        plan.process(xd, out, T, B, 0, B)

    graph = capture_on_side_stream(record)
    assert (plan.form(T, B), plan.form(T, 1)) == was
    assert same(host(out), ref) and same(host(plan.pressure()), grids[0])
    assert not host(fresh.pressure()).any()
    for k in range(2):
        graph.replay()
        orc.fdtd(P, grids, x, ref, T, B, 0, B, fused=True)
        torch.cuda.synchronize()
        assert same(host(out), ref), k
        assert same(host(plan.pressure()), grids[0]), k
    # outside a capture both calls are served: an odd one, and one that grows the strips
    orc.fdtd(P, grids, x, ref, T, B, 0, 1, fused=True)
    plan.process(xd, out, T, B, 0, 1)
    assert same(host(out), ref) and same(host(plan.pressure()), grids[0])
    plan.process(x2, out2, T, 2 * B, 0, 2 * B)
    torch.cuda.synchronize()
    del graph
    plan.close()
    fresh.close()


# =====================================================================================================================
# Waveguides
# =====================================================================================================================
ML = 2000


def dwg_bank(orc, n, B):
    """Taps that are really reached (the reference's placement never is) and write positions spread over the lines."""
    wg, x = orc.dwg_init(n, B)
    L = wg["length"].astype(np.int64)
    wg["writePos"] = (np.arange(n) * 13) % L
    wg["outputTapPos"] = wg["inputTapPos"] = (wg["writePos"] + (np.arange(n) % 5) * 3) % L
    return wg, x


# (cells, mix) -> (n, B, out_tracks, variant)
#   sparse mix: min(n, out_tracks) >= 2048;  lean: sparse and B <= 2048 (four lines per workgroup: n % 4 != 0 is ragged);
#   multi: n >= 1024 otherwise;  one_line below;  the input is staged in LDS up to B = 2048 and read from memory above
DWG_SHAPES = {
    ("naive", "scan"): [(40, 300, 40, "naive")],
    ("naive", "gather_sparse"): [(2049, 64, 2049, "naive")],
    ("one_line", "scan"): [(40, 2100, 40, "accel")],
    ("multi", "scan"): [(1030, 300, 1030, "accel"), (1024, 2000, 1024, "accel"), (2050, 256, 100, "accel"),
                        (1500, 2100, 1500, "accel")],
    ("multi", "gather_sparse"): [(2051, 2049, 2051, "accel")],
    ("lean", "appended_sparse"): [(2049, 384, 2049, "accel"), (2051, 100, 2051, "accel"), (2050, 2048, 2050, "accel")],
}
DWG_CASES = [(c, m) + shape for (c, m), shapes in DWG_SHAPES.items() for shape in shapes]
# The form for delay lines of 4 GiB and more per array is asked, not run (no test allocates two such arrays).
DWG_ASKED_ONLY = {("append_staged", "appended_sparse"): (2148, 512, 500000, 2148, "accel")}


@pytest.mark.parametrize("cells,mix,n,B,out_tracks,variant", DWG_CASES,
                         ids=["%s-%s-%d-%d-%d" % c[:5] for c in DWG_CASES])
def test_dwg_route(gab, orc, cells, mix, n, B, out_tracks, variant):
    """A bank per route of gab_dwg: mix and both delay-line banks bit for bit the oracle's over four buffers on one state."""
    import torch
    v = gab.DWG_NAIVE if variant == "naive" else gab.DWG_ACCEL
    assert gab.dwg_route(n, B, ML, out_tracks, v) == (cells, mix)
    wg, x = dwg_bank(orc, n, B)
    fwd_r, bwd_r = np.zeros(n * ML, np.float32), np.zeros(n * ML, np.float32)
    fwd, bwd = torch.zeros(n * ML, device="cuda"), torch.zeros(n * ML, device="cuda")
    wg_d, xd = dev(wg.view(np.uint8)), dev(x)
    for it in range(4):
        y = host(gab.dwg(wg_d, fwd, bwd, xd, B, ML, out_tracks=out_tracks, variant=v))
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML, out_tracks=out_tracks)
        assert same(y, ry), it
        assert same(host(fwd), fwd_r), it
        assert same(host(bwd), bwd_r), it
    assert np.count_nonzero(ry) >= 3 and fwd_r.any() and bwd_r.any()


def test_dwg_route_asked_only(gab):
    for (cells, mix), (n, B, max_len, out_tracks, variant) in DWG_ASKED_ONLY.items():
        assert gab.dwg_route(n, B, max_len, out_tracks, gab.DWG_ACCEL) == (cells, mix)
        assert gab.dwg_route(n, B, max_len - 1000, out_tracks, gab.DWG_ACCEL) == ("lean", mix)


def test_dwg_more_calls_in_flight_than_counter_slots(gab, orc):
    """The lean route keeps its per-sample counters in one of 16 slots of the library, taken round robin; a slot's event
    orders a call behind the slot's last user on another stream.  18 calls on three streams, round robin, no host wait
    in between: every stream's bank ends where the oracle's is after six buffers."""
    import torch
    n, B, streams, per_stream = 2048, 128, 3, 6
    assert gab.dwg_route(n, B, ML, n) == ("lean", "appended_sparse")
    wg, x = dwg_bank(orc, n, B)
    fwd_r, bwd_r = np.zeros(n * ML, np.float32), np.zeros(n * ML, np.float32)
    for it in range(per_stream):
        ry = orc.dwg(wg, fwd_r, bwd_r, x, B, ML, out_tracks=n)
    assert np.count_nonzero(ry) >= 3
    wg_d, xd = dev(wg.view(np.uint8)), dev(x)
    banks = [(torch.zeros(n * ML, device="cuda"), torch.zeros(n * ML, device="cuda")) for _ in range(streams)]
    ss = [torch.cuda.Stream() for _ in range(streams)]
    torch.cuda.synchronize()
    last = [None] * streams
    for it in range(per_stream):
        for k in range(streams):
            with torch.cuda.stream(ss[k]):
                last[k] = gab.dwg(wg_d, banks[k][0], banks[k][1], xd, B, ML, out_tracks=n, variant=gab.DWG_ACCEL)
    torch.cuda.synchronize()
    for k in range(streams):
        assert same(host(last[k]), ry), k
        assert same(host(banks[k][0]), fwd_r), k
        assert same(host(banks[k][1]), bwd_r), k


# =====================================================================================================================
# Modal bank
# =====================================================================================================================
# (J, fixed_tracks) -> (n_modes, bufsize, tracks).  J doubles while ceil(rows / (8 * slots * J)) > 256 workgroups, with
# rows = ceil(n_modes / tracks) and slots = 64 // tracks; up to 8 with 32 tracks (compile-time count), up to 4 otherwise.
MODAL_SHAPES = {
    (1, 1): [(3000, 20, 32)],
    (2, 1): [(140000, 20, 32)],
    (4, 1): [(300001, 20, 32)],                        # ragged last row, partial chunk
    (8, 1): [(1 << 20, 20, 32)],
    (1, 0): [(3333, 20, 7)],
    (2, 0): [(98305 + 24 * 5, 20, 24), (140000, 16, 7), (140000, 20, 1)],
    (4, 0): [(200000, 17, 24), (270000, 33, 7), (270001, 20, 64)],
}
MODAL_CASES = [form + shape for form, shapes in MODAL_SHAPES.items() for shape in shapes]
MODAL_IDS = ["J%d-%s-%d-%d-%d" % (c[0], "fixed" if c[1] else "rt", c[2], c[3], c[4]) for c in MODAL_CASES]


@pytest.mark.parametrize("J,fixed,n_modes,bufsize,tracks", MODAL_CASES, ids=MODAL_IDS)
def test_modal_launch_form_sums(gab, orc, J, fixed, n_modes, bufsize, tracks):
    """The project's gate on the sums (1e-5 of the float64-accumulated peak, against both references) per instantiation."""
    assert gab.modal_launch(n_modes, tracks)[::2] == (J, fixed)
    p = orc.modal_params(n_modes)
    y = host(gab.modal_bank(dev(p), n_modes, bufsize, tracks))
    ref = orc.modal_bank(p, n_modes, bufsize, tracks)
    ref64 = orc.modal_bank_f64acc(p, n_modes, bufsize, tracks)
    peak = np.abs(ref64).max()
    assert peak > 0
    assert np.abs(y - ref64).max() <= 1e-5 * peak
    assert np.abs(y - ref).max() <= 1e-5 * peak


def one_hot_modes(n_modes, tracks, J, grid):
    """Modes at the corners of the kernel's layout (k_modal.hip): 64 // tracks slots of a wave serve each track, lane =
    slot * tracks + track; wave w of workgroup g owns rows [(8 g + w) * slots * J, + slots * J) of `tracks` modes each,
    and lane (slot, track) holds in register j the mode (first_row + j * slots + slot) * tracks + track."""
    slots, waves = 64 // tracks, 8

    def mode(g, w, j, slot, track):
        return (((g * waves + w) * slots * J) + j * slots + slot) * tracks + track

    picks = {
        "mode_0": 0,
        "last_mode": n_modes - 1,
        "last_register_of_the_last_workgroup": mode(grid - 1, 0, J - 1, 0, 0),
        "first_of_workgroup_1": mode(1, 0, 0, 0, 0),
        "highest_slot": mode(0, waves - 1, J - 1, slots - 1, tracks - 1),
    }
    assert all(0 <= m < n_modes for m in picks.values()), picks
    assert mode(grid, 0, 0, 0, 0) >= n_modes > mode(grid - 1, 0, 0, 0, 0)        # the grid covers the modes, no more
    return picks


ONE_HOT_CASES = [c for c in MODAL_CASES if c[0] >= 2]


@pytest.mark.parametrize("J,fixed,n_modes,bufsize,tracks", ONE_HOT_CASES,
                         ids=[i for i, c in zip(MODAL_IDS, MODAL_CASES) if c[0] >= 2])
def test_modal_one_mode_alone_is_its_own_sequence_on_its_own_track(gab, orc, J, fixed, n_modes, bufsize, tracks):
    """Every amplitude zero but one mode's: the sum holds that mode's sequence and zeros, and adding zeros is exact, so
    the output is the oracle's bit for bit (up to the sign of a zero) — on track mode % tracks, nothing anywhere else.
    A lane that holds another mode in register j than the layout says cannot pass this."""
    J_, grid, fixed_ = gab.modal_launch(n_modes, tracks)
    assert (J_, fixed_) == (J, fixed)
    base = orc.modal_params(n_modes).reshape(n_modes, 8)
    for name, m in one_hot_modes(n_modes, tracks, J, grid).items():
        q = base.copy()
        amp = q[m, 0] if q[m, 0] != 0 else np.float32(0.5)
        q[:, 0] = 0.0
        q[m, 0] = amp
        y = host(gab.modal_bank(dev(q.ravel()), n_modes, bufsize, tracks)).reshape(tracks, bufsize)
        ref = orc.modal_bank(q.ravel(), n_modes, bufsize, tracks).reshape(tracks, bufsize)
        assert same(np.abs(y), np.abs(ref)), (name, m)
        assert np.count_nonzero(ref[m % tracks]) >= bufsize - 1, (name, m)
        others = np.delete(np.arange(tracks), m % tracks)
        assert not y[others].any() and not ref[others].any(), (name, m)


# =====================================================================================================================
# The census
# =====================================================================================================================
def test_every_form_of_the_three_queries_has_a_case(gab):
    """The lists above against the enumerators of the queries: a form added to a dispatcher has no case here until
    somebody writes one, and this fails until then."""
    assert set(FDTD_ROOMS) == set(gab.FDTD_FORMS) and all(FDTD_ROOMS[f] for f in gab.FDTD_FORMS)
    assert set(b for a, b in CAPTURE_ROOMS.values()) <= set(gab.FDTD_FORMS)
    cells_run = set(c for c, m in DWG_SHAPES if DWG_SHAPES[(c, m)])
    mixes_run = set(m for c, m in DWG_SHAPES if DWG_SHAPES[(c, m)])
    assert cells_run | set(c for c, m in DWG_ASKED_ONLY) == set(gab.DWG_CELLS)
    assert set(c for c, m in DWG_ASKED_ONLY) == {"append_staged"}            # 4 GiB of lines: asked, never allocated
    assert mixes_run == set(gab.DWG_MIX)
    assert set(MODAL_SHAPES) == set(gab.MODAL_FORMS) and all(MODAL_SHAPES[f] for f in gab.MODAL_FORMS)
    assert set(c[:2] for c in ONE_HOT_CASES) == set(f for f in gab.MODAL_FORMS if f[0] >= 2)
