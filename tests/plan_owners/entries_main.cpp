// The entry bodies of gab_plan.hpp (create_entry, entry, batch_entry, expose_entry, row_refusal, overlaps, all_aligned16,
// ring_capacity, DeviceBuf::fill) with a small fake plan, against the counting stubs of the runtime beside this file,
// for a host compiler with -fsanitize=address,undefined: what each refusal says and returns, in which order the checks
// run, that *out is null after every create that did not succeed and that nothing of it stays behind.  Built and run by
// tests/test_plan_owners_host.py.
#include <cstdio>
#include <stdexcept>
#include <string>

#include "gab_plan.hpp"

static std::string g_error;
static bool g_mode_refused = false;
namespace gab {                         // (gab_runtime.cpp's, which is not linked here)
void set_last_error(const std::string& msg) { g_error = msg; }
const char* last_error() { return g_error.c_str(); }
int refuse_unsupported_runtime_mode(const char* who) {
    if (!g_mode_refused) return GAB_OK;
    set_last_error(std::string(who) + ": the runtime mode is not supported");
    return GAB_ERR_UNSUPPORTED;
}
}  // namespace gab

static int g_failed = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("%s:%d: expected %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

static bool said(int rc, int code, const char* text) {
    if (rc == code && g_error == text) return true;
    std::printf("  got %d \"%s\"\n", rc, g_error.c_str());
    return false;
}

struct Fake {
    int tracks = 0, bufsize = 0, odd = 0;
    gab::RampedTable params;            // [tracks][2]
    gab::DeviceBuf<int> count;          // [tracks]
};

static long live_all() {
    long n = 0;
    for (int k = 0; k < stub::kKinds; ++k) n += (long)stub::state().live[k].size();
    return n;
}

static int g_checks = 0, g_builds = 0;

// a create as a plan file writes it; status: what its build returns
static int fake_create(Fake** out, int tracks, int bufsize, int odd, int status = GAB_OK) {
    return gab::create_entry("fake_create", out, tracks, bufsize, [&] {
        ++g_checks;
        if (odd % 2 == 0) return gab::bad_arg("fake_create: odd must be odd");
        return GAB_OK;
    }, [&](Fake& p) {
        ++g_builds;
        p.odd = odd;
        p.params.create((size_t)tracks * 2, bufsize);      // three device allocations
        p.params.fill({0.5f, -1.0f}, tracks);
        p.count.alloc((size_t)tracks);                     // the fourth
        p.count.fill(-1);
        return status;
    });
}

int main() {
    Fake* const stale = reinterpret_cast<Fake*>(0x10);
    Fake* f = stale;

    // ---- create ----
    EXPECT(said(fake_create(nullptr, 3, 8, 1), GAB_ERR_INVALID_ARG, "fake_create: null plan pointer"));
    EXPECT(g_checks == 0 && g_builds == 0);
    EXPECT(said(fake_create(&f, 0, 8, 1), GAB_ERR_INVALID_ARG, "fake_create: tracks and bufsize must be > 0") && !f);
    f = stale;
    EXPECT(said(fake_create(&f, 3, -1, 1), GAB_ERR_INVALID_ARG, "fake_create: tracks and bufsize must be > 0") && !f);
    EXPECT(g_checks == 0 && g_builds == 0);                // the shape is judged before the plan's own check
    f = stale;
    g_mode_refused = true;                                 // the plan's own check comes before the runtime mode's
    EXPECT(said(fake_create(&f, 3, 8, 2), GAB_ERR_INVALID_ARG, "fake_create: odd must be odd") && !f);
    EXPECT(g_checks == 1 && g_builds == 0);
    f = stale;
    EXPECT(said(fake_create(&f, 3, 8, 1), GAB_ERR_UNSUPPORTED, "fake_create: the runtime mode is not supported") && !f);
    EXPECT(g_checks == 2 && g_builds == 0 && live_all() == 0);
    g_mode_refused = false;
    for (int at = 0; at < 4; ++at) {                       // a throw at every one of the build's four allocations
        f = stale;
        stub::fail_after(at);
        EXPECT(fake_create(&f, 3, 8, 1) == GAB_ERR_RUNTIME && !f && live_all() == 0);
    }
    stub::fail_after(-1);
    EXPECT(g_builds == 4);
    f = stale;
    EXPECT(fake_create(&f, 3, 8, 1, 77) == 77 && !f && live_all() == 0);   // a build that returns a launch's status
    f = stale;
    EXPECT(fake_create(&f, 3, 8, 1) == GAB_OK && f && f != stale);
    EXPECT(f->tracks == 3 && f->bufsize == 8 && f->odd == 1 && live_all() == 4);
    EXPECT(f->count.size() == 3 && f->count.get()[0] == -1 && f->count.get()[2] == -1);            // DeviceBuf::fill
    EXPECT(f->params.target.get()[4] == 0.5f && f->params.current.get()[5] == -1.0f);

    // ---- the exposed table ----
    float *cur = nullptr, *tgt = nullptr;
    size_t n = 0;
    EXPECT(said(gab::expose_entry("fake_params", f, &Fake::params, nullptr, &tgt, &n), GAB_ERR_INVALID_ARG,
                "fake_params: null pointer"));
    EXPECT(said(gab::expose_entry("fake_params", (Fake*)nullptr, &Fake::params, &cur, &tgt, &n), GAB_ERR_INVALID_ARG,
                "fake_params: null pointer"));
    EXPECT(!cur && !tgt && n == 0);
    EXPECT(gab::expose_entry("fake_params", f, &Fake::params, &cur, &tgt, &n) == GAB_OK);
    EXPECT(cur == f->params.current.get() && tgt == f->params.target.get() && n == 6);

    // ---- process, process_batch and the calls that only check for null ----
    int ran = 0;
    auto body = [&] { ++ran; return 5; };
    float x = 0.0f;
    EXPECT(said(gab::entry("fake_process", {f, nullptr, &x}, body), GAB_ERR_INVALID_ARG, "fake_process: null pointer"));
    EXPECT(said(gab::entry("fake_reset", {nullptr}, body, "null plan"), GAB_ERR_INVALID_ARG, "fake_reset: null plan"));
    EXPECT(ran == 0);
    EXPECT(gab::entry("fake_process", {f, &x, &x}, body) == 5 && ran == 1);
    EXPECT(said(gab::batch_entry("fake_process_batch", {f, nullptr, &x}, 0, body), GAB_ERR_INVALID_ARG,
                "fake_process_batch: null pointer"));      // null, then n_buffers
    EXPECT(said(gab::batch_entry("fake_process_batch", {f, &x, &x}, 0, body), GAB_ERR_INVALID_ARG,
                "fake_process_batch: n_buffers must be > 0"));
    EXPECT(said(gab::batch_entry("fake_process_batch", {f, &x, &x}, -3, body), GAB_ERR_INVALID_ARG,
                "fake_process_batch: n_buffers must be > 0"));
    EXPECT(ran == 1);                                      // no body after a refusal
    EXPECT(gab::batch_entry("fake_process_batch", {f, &x, &x}, 2, body) == 5 && ran == 2);
    EXPECT(said(gab::batch_entry("fake_process_batch", {f, &x, &x}, 1, [&]() -> int {     // the body's own refusal
        return gab::refuse("fake_process_batch", "d_key may not overlap d_out");
    }), GAB_ERR_INVALID_ARG, "fake_process_batch: d_key may not overlap d_out"));
    EXPECT(said(gab::entry("fake_process", {f}, [&]() -> int { throw std::runtime_error("hipLaunch: stub error"); }),
                GAB_ERR_RUNTIME, "hipLaunch: stub error"));

    // ---- destroy: creates equal destroys ----
    EXPECT(said(gab::destroy_plan((Fake*)nullptr, "fake_destroy: null pointer"), GAB_ERR_INVALID_ARG,
                "fake_destroy: null pointer"));
    EXPECT(gab::destroy_plan(f, "fake_destroy: null pointer") == GAB_OK && live_all() == 0);
    for (int k = 0; k < stub::kKinds; ++k) EXPECT(stub::state().creates[k] == stub::state().destroys[k]);
    EXPECT(stub::state().creates[stub::kDevice] == 4 + (0 + 1 + 2 + 3) + 4 && stub::state().bad_destroys == 0);

    // ---- the text of a row rule: a field in the middle of the second row, first_track = 5 (delay, dynamics, gate,
    //      reverb with four lines and one output: 17 floats a row) ----
    EXPECT(gab::row_refusal(4 + 2, 4, 5, "wet", "must be finite") ==
           "track 6 field 2 (wet) must be finite; the plan keeps its parameters");
    EXPECT(gab::row_refusal(8 + 4, 8, 5, "att", "must be within [0, 1 - 2^-20]") ==
           "track 6 field 4 (att) must be within [0, 1 - 2^-20]; the plan keeps its parameters");
    EXPECT(gab::row_refusal(7 + 3, 7, 5, "rel", "must be within [0, 1 - 2^-20]") ==
           "track 6 field 3 (rel) must be within [0, 1 - 2^-20]; the plan keeps its parameters");
    EXPECT(gab::row_refusal(17 + 5, 17, 5, "damp", "must be within [0, 1 - 2^-20]") ==
           "track 6 field 5 (damp) must be within [0, 1 - 2^-20]; the plan keeps its parameters");
    EXPECT(gab::row_refusal(0, 4, 0, "delay", "r") == "track 0 field 0 (delay) r; the plan keeps its parameters");

    // ---- pointers ----
    alignas(16) float a[16] = {};
    EXPECT(!gab::overlaps(a, a + 4, 4) && !gab::overlaps(a + 4, a, 4));        // touching
    EXPECT(gab::overlaps(a, a + 3, 4) && gab::overlaps(a + 3, a, 4));          // by one float
    EXPECT(gab::overlaps(a, a, 1) && gab::overlaps(a + 1, a, 8));              // the same, nested
    EXPECT(!gab::overlaps(a, a + 12, 4) && !gab::overlaps(a + 12, a, 4));      // disjoint
    EXPECT(gab::all_aligned16({a, a + 4, nullptr}) && !gab::all_aligned16({a, a + 1}) && !gab::all_aligned16({a + 2}));
    EXPECT(gab::ring_capacity(1) == 1 && gab::ring_capacity(2) == 2 && gab::ring_capacity(3) == 4);
    EXPECT(gab::ring_capacity(64) == 64 && gab::ring_capacity(65) == 128);
    EXPECT(gab::ring_capacity(((size_t)1 << 20) + 3 + 8) == (size_t)1 << 21);

    if (g_failed) {
        std::printf("plan entries: %d expectation(s) failed\n", g_failed);
        return 1;
    }
    std::printf("plan entries ok: %ld device allocations made and freed once each, %d checks, %d builds\n",
                stub::state().creates[stub::kDevice], g_checks, g_builds);
    return 0;
}
