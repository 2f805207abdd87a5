"""Host cost of plan.launch(args): wall-clock per call over 20 000 calls, T = B = 64, one synchronise at the end.
The plans' per-call path of a real-time loop is launch(args) = check(fn(*args)); the device work is small, so what is
timed is the host: ctypes, the entry's checks, the launch.  Every call is timed on its own (the median does not see the
calls that wait for a full queue; the loop's mean does).

    python tools/plan_launch_cost.py <root that holds gpuaudiobench_amd, built> <label>

To compare two commits, run it on a checkout of each on the same machine, one after the other: A, B, A."""
import statistics
import sys
import time

sys.path.insert(0, sys.argv[1])
import torch  # noqa: E402
import gpuaudiobench_amd as gab  # noqa: E402

assert gab.__file__.startswith(sys.argv[1]), gab.__file__
T = B = 64
N = 20000


def measure(name, plan, args):
    launch = plan.launch
    for _ in range(500):
        launch(args)
    torch.cuda.synchronize()
    clock = time.perf_counter_ns
    ts = [0] * N
    t_all = clock()
    for i in range(N):
        t0 = clock()
        launch(args)
        ts[i] = clock() - t0
    t_all = clock() - t_all
    torch.cuda.synchronize()
    ts.sort()
    print("%-8s %-22s median %7.0f ns  p10 %7.0f  p90 %7.0f  mean(loop) %7.0f ns" % (
        sys.argv[2], name, statistics.median(ts), ts[N // 10], ts[9 * N // 10], t_all / N), flush=True)


x = torch.randn(T * B, device="cuda")
key = torch.randn(T * B, device="cuda")
out = torch.empty_like(x)
act = torch.zeros(T, dtype=torch.int32, device="cuda")
d = gab.DelayPlan(T, B, 64)
measure("DelayPlan", d, d.prepare(x, out))
y = gab.DynamicsPlan(T, B)
measure("DynamicsPlan key", y, y.prepare(x, out, key=key))
g = gab.GatePlan(T, B)
measure("GatePlan key act", g, g.prepare(x, out, key=key, act=act))
