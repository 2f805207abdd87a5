// The owners of gab_plan.hpp (DeviceBuf, PinnedBuf, Event, Stream) against counting stubs of the runtime
// (hip/hip_runtime.h beside this file), for a host compiler with -fsanitize=address,undefined: every create is
// matched by one destroy, nothing is destroyed twice, and a create that fails half-way through a struct held in a
// unique_ptr takes the first half with it.  Built and run by tests/test_plan_owners_host.py.
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>

#include "gab_plan.hpp"

namespace gab {                         // (gab_runtime.cpp's, which is not linked here)
void set_last_error(const std::string&) {}
const char* last_error() { return ""; }
}  // namespace gab

static int g_failed = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("%s:%d: expected %s\n", __FILE__, __LINE__, #cond);   \
            ++g_failed;                                                       \
        }                                                                     \
    } while (0)

static long live(stub::Kind k) { return (long)stub::state().live[k].size(); }
static long creates(stub::Kind k) { return stub::state().creates[k]; }
static long destroys(stub::Kind k) { return stub::state().destroys[k]; }

// make(o) brings an empty owner to life; the same walk for all four kinds
template <class Owner, class Make>
static void walk(stub::Kind k, Make make) {
    const long c0 = creates(k), d0 = destroys(k);
    {
        Owner a;
        EXPECT(!a && a.get() == nullptr);
        make(a);
        EXPECT(a && live(k) == 1);
        auto* const first = a.get();

        Owner b(std::move(a));                      // move-construct: one handle, now b's
        EXPECT(!a && b.get() == first && live(k) == 1);

        Owner c;
        make(c);
        auto* const second = c.get();
        EXPECT(live(k) == 2);
        c = std::move(b);                           // move-assign onto a live one: c's old handle goes with b
        EXPECT(c.get() == first && live(k) == 2);
        b.release();
        EXPECT(!b && live(k) == 1 && stub::state().live[k].count(second) == 0);

        c = std::move(c);                           // onto itself: nothing moves, nothing goes
        EXPECT(c.get() == first && live(k) == 1);

        bool refused = false;                       // a second create on a live owner would leak the first
        try { make(c); } catch (const std::logic_error&) { refused = true; }
        EXPECT(refused && c.get() == first && live(k) == 1);

        c.release();                                // release and re-create
        EXPECT(!c && live(k) == 0);
        c.release();                                // (twice is once)
        make(c);
        EXPECT(c && live(k) == 1);

        Owner d;
        make(d);
        auto* const pc = c.get();
        auto* const pd = d.get();
        c.swap(d);
        EXPECT(c.get() == pd && d.get() == pc && live(k) == 2);
        c.swap(c);                                  // self-swap
        EXPECT(c.get() == pd && live(k) == 2);
        Owner e;
        e.swap(c);                                  // with an empty one
        EXPECT(!c && e.get() == pd && live(k) == 2);

        stub::fail_after(0);                        // a create that fails leaves the owner empty
        Owner f;
        bool threw = false;
        try { make(f); } catch (const std::runtime_error&) { threw = true; }
        EXPECT(threw && !f && live(k) == 2);
    }
    EXPECT(live(k) == 0);
    EXPECT(creates(k) - c0 == destroys(k) - d0);
    EXPECT(creates(k) - c0 == 4);                   // a, c, c again, d (the refused and the failed one made nothing)
}

// A plan's lazily made state as the plans write it: several owners in a struct, built by a function that returns it whole
// or throws, the struct in a unique_ptr.
struct Whole {
    gab::DeviceBuf<unsigned> stage;
    gab::DeviceBuf<float> park;
    gab::Event check_ev[2];
    gab::PinnedBuf<unsigned> words;
    gab::Stream copy_stream;
    gab::Event copy_ev;
};

static std::unique_ptr<Whole> make_whole() {
    std::unique_ptr<Whole> w(new Whole);
    w->stage.alloc_with_flags(64, hipDeviceMallocFinegrained);
    w->park.alloc(32);
    for (gab::Event& e : w->check_ev) e.create();
    w->words.alloc(64);
    w->copy_stream = gab::Stream::highest_priority();
    w->copy_ev.create();
    return w;
}

static long live_all() {
    long n = 0;
    for (int k = 0; k < stub::kKinds; ++k) n += live((stub::Kind)k);
    return n;
}

int main() {
    walk<gab::DeviceBuf<float>>(stub::kDevice, [](gab::DeviceBuf<float>& b) { b.alloc(16); });
    walk<gab::DeviceBuf<unsigned>>(stub::kDevice, [](gab::DeviceBuf<unsigned>& b) { b.alloc_with_flags(16, hipDeviceMallocDefault); });
    walk<gab::PinnedBuf<unsigned>>(stub::kPinned, [](gab::PinnedBuf<unsigned>& b) { b.alloc(64); });
    walk<gab::Event>(stub::kEvent, [](gab::Event& e) { e.create(); });
    walk<gab::Stream>(stub::kStream, [](gab::Stream& s) { s.create(hipStreamNonBlocking); });
    walk<gab::Stream>(stub::kStream, [](gab::Stream& s) {
        if (s) throw std::logic_error("the maker has no live stream to refuse: this walk does");
        s = gab::Stream::highest_priority();
    });

    {   // sizes, and pinned memory comes zeroed and is the host's to write
        gab::DeviceBuf<float> d;
        d.alloc(7);
        EXPECT(d.size() == 7);
        d.release();
        EXPECT(d.size() == 0);
        gab::PinnedBuf<unsigned> w;
        w.alloc(64);
        unsigned sum = 0;
        for (size_t i = 0; i < w.size(); ++i) sum |= w[i];
        EXPECT(sum == 0 && w.size() == 64);
        w[63] = 5;
        EXPECT(w.get()[63] == 5);
    }

    // the struct whole: seven creates, and all of them go with it
    {
        std::unique_ptr<Whole> held;
        EXPECT(!held);
        held = make_whole();
        EXPECT(held && live_all() == 7);
    }
    EXPECT(live_all() == 0);
    // a throw at every one of its seven creates in turn: the holder stays empty and nothing stays behind
    for (int at = 0; at < 7; ++at) {
        std::unique_ptr<Whole> held;
        stub::fail_after(at);
        bool threw = false;
        try { held = make_whole(); } catch (const std::runtime_error&) { threw = true; }
        EXPECT(threw && !held);
        EXPECT(live_all() == 0);
    }
    stub::fail_after(-1);

    // a resized pair (the engine's rings): the old pair goes, the new one is made aside and moved in only when both exist
    {
        gab::DeviceBuf<float> in, out;
        in.alloc(8);
        out.alloc(8);
        in.release();
        out.release();
        stub::fail_after(1);                        // the second of the new pair fails
        bool threw = false;
        try {
            gab::DeviceBuf<float> a, b;
            a.alloc(16);
            b.alloc(16);
            in = std::move(a);
            out = std::move(b);
        } catch (const std::runtime_error&) { threw = true; }
        EXPECT(threw && !in && !out && live(stub::kDevice) == 0);
    }

    for (int k = 0; k < stub::kKinds; ++k) {
        EXPECT(live((stub::Kind)k) == 0);
        EXPECT(creates((stub::Kind)k) == destroys((stub::Kind)k));
        EXPECT(creates((stub::Kind)k) > 0);
    }
    EXPECT(stub::state().bad_destroys == 0);
    if (g_failed) {
        std::printf("plan owners: %d expectation(s) failed\n", g_failed);
        return 1;
    }
    std::printf("plan owners ok: %ld device, %ld pinned, %ld event, %ld stream handles made and destroyed once each\n",
                creates(stub::kDevice), creates(stub::kPinned), creates(stub::kEvent), creates(stub::kStream));
    return 0;
}
