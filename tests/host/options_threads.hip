// Stand-alone host program: the option scope (csrc/options.hip) under real threads.  Links options.hip and nothing else of the engine,
// never touches a device.  Built and run by tests/test_threads_cpu.py (with a host sanitizer where the toolchain ships one); exit status
// 0 = every check held.  Every loop has a fixed length or ends on a hand-shake: nothing here is judged on timing.
//
//   1 snapshot constancy   every re-read inside one LtOptScope equals the first read, whatever the setters do meanwhile
//   2 ordering rule        value written first, generation bumped second, generation READ first: a snapshot never holds an older value
//                          under a newer generation (process defaults, the engine slot + gen, and lt_opt_reset_process)
//   3 locality / nesting   a scope is visible on its own thread only; a nested scope restores the outer one, generations included
//   4 override resolution  an engine slot flipped between a value and LT_OPT_INHERIT: a snapshot holds that value or a process default
#include <atomic>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <thread>
#include <vector>

#include "options.h"

// options.hip's one reference into the engine (lt_opt_validate reports through it; nothing here validates)
void lt_set_error(const char*, ...) {}

namespace {
std::atomic<long> g_failures{0};

void fail(const char* fmt, ...) {
    if (g_failures.fetch_add(1) >= 20) return;  // (the first few say it all)
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "FAIL: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
}
#define CHECK(cond, ...) do { if (!(cond)) fail(__VA_ARGS__); } while (0)

// what lt_engine_set_option does to an engine's options (csrc/engine.hip): the slot, then the generation
void engine_set(LtEngineOptions& o, int id, int value) {
    o.v[id].store(value, std::memory_order_relaxed);
    o.gen.fetch_add(1, std::memory_order_release);
}

struct Lcg {
    unsigned s;
    unsigned next() { s = s * 1664525u + 1013904223u; return s >> 8; }
};

void run_all(std::vector<std::function<void()>> fns) {
    std::vector<std::thread> th;
    for (auto& f : fns) th.emplace_back(f);
    for (auto& t : th) t.join();
}

// ---- 1 ------------------------------------------------------------------------------------------------------------------------
void check_constancy() {
    constexpr int READERS = 4, SCOPES = 4000, REREADS = 4;
    LtEngineOptions eng;
    std::atomic<int> readers_left{READERS};
    std::atomic<long> changed{0};  // scopes whose generation differed from the scope before: the setters really ran underneath
    auto setter = [&](unsigned seed) {
        Lcg r{seed};
        for (long i = 0; readers_left.load() > 0; ++i) {
            const int id = (int)(r.next() % LT_OPT_COUNT);
            const LtOptDesc& d = kLtOptDesc[id];
            const int v = d.lo + (int)(r.next() % (unsigned)(d.hi - d.lo + 1));
            lt_opt_set_process(id, v);
            engine_set(eng, id, r.next() % 3 == 0 ? LT_OPT_INHERIT : v);
            if (i % 64 == 63) lt_opt_reset_process();
        }
    };
    auto reader = [&](const LtEngineOptions* o) {
        int last_gen = -1;
        for (int k = 0; k < SCOPES; ++k) {
            LtOptScope scope(o);
            int first[LT_OPT_COUNT];
            for (int i = 0; i < LT_OPT_COUNT; ++i) first[i] = lt_opt(i);
            const int pg = lt_opt_generation(), eg = lt_opt_engine_generation();
            if (pg != last_gen) changed.fetch_add(1);
            last_gen = pg;
            CHECK(o || eg == 0, "constancy: engine generation %d in a scope without an engine", eg);
            for (int rep = 0; rep < REREADS; ++rep) {
                for (int i = 0; i < LT_OPT_COUNT; ++i) {
                    const int v = lt_opt(i);
                    CHECK(v == first[i], "constancy: option %s read %d, then %d inside one scope", kLtOptDesc[i].name, first[i], v);
                }
                CHECK(lt_opt_generation() == pg && lt_opt_engine_generation() == eg, "constancy: a generation moved inside one scope");
                std::this_thread::yield();
            }
        }
        readers_left.fetch_sub(1);
    };
    run_all({[&] { setter(1); }, [&] { setter(2); }, [&] { reader(&eng); }, [&] { reader(&eng); }, [&] { reader(nullptr); },
             [&] { reader(nullptr); }});
    lt_opt_reset_process();
    printf("constancy: %d scopes x %d re-reads of %d options; %ld scopes opened on a generation the previous one had not seen\n",
           READERS * SCOPES, REREADS, (int)LT_OPT_COUNT, changed.load());
}

// ---- 2 ------------------------------------------------------------------------------------------------------------------------
// One round: the setter writes 1, 2, .. STEPS into gemm_stagger (range 0..256: no wrap), each followed by one generation bump, so after
// step i the generation stands at g0 + i.  A snapshot that reads the generation first sees value >= generation - g0.  The setter takes its
// next step once a reader has opened another scope: every value is looked at, and no reader ever waits.
void check_ordering(bool engine_slot) {
    constexpr int ROUNDS = 100, STEPS = 256, READERS = 2;
    static_assert(STEPS <= 256, "gemm_stagger holds 0 .. 256");
    long snapshots = 0, newer_value = 0;
    for (int round = 0; round < ROUNDS; ++round) {
        LtEngineOptions eng;
        lt_opt_set_process(OPT_GEMM_STAGGER, 0);
        const int g0 = engine_slot ? 0 : lt_opt_generation();
        std::atomic<long> snaps{0}, newer{0};
        std::atomic<bool> done{false}, reset_started{false};
        auto reader = [&] {
            while (!done.load()) {
                int v, d;
                {
                    LtOptScope scope(engine_slot ? &eng : nullptr);
                    v = lt_opt(OPT_GEMM_STAGGER);
                    d = (engine_slot ? lt_opt_engine_generation() : lt_opt_generation()) - g0;
                }
                // (the process round ends on lt_opt_reset_process, step STEPS + 1: the default, 0, is the newest value then)
                std::atomic_thread_fence(std::memory_order_seq_cst);  // (pairs with the setter's: a 0 read from the reset sees the flag too)
                const bool is_reset_value = !engine_slot && v == 0 && reset_started.load();
                if (d <= STEPS) CHECK(v >= d || is_reset_value, "ordering (%s): value %d under generation offset %d - an older value under a newer generation",
                                      engine_slot ? "engine" : "process", v, d);
                else CHECK(v == 0, "ordering (reset): value %d under the generation lt_opt_reset_process left", v);
                CHECK(d >= 0 && d <= STEPS + 1 && v >= 0 && v <= STEPS, "ordering: value %d / generation offset %d outside the round", v, d);
                if (v > d) newer.fetch_add(1);
                snaps.fetch_add(1);
            }
        };
        auto setter = [&] {
            for (int i = 1; i <= STEPS; ++i) {
                const long seen = snaps.load();
                if (engine_slot) engine_set(eng, OPT_GEMM_STAGGER, i);
                else lt_opt_set_process(OPT_GEMM_STAGGER, i);
                while (snaps.load() == seen) std::this_thread::yield();
            }
            if (!engine_slot) {
                const long seen = snaps.load();
                reset_started.store(true);
                std::atomic_thread_fence(std::memory_order_seq_cst);
                lt_opt_reset_process();
                while (snaps.load() == seen) std::this_thread::yield();
            }
            done.store(true);
        };
        std::vector<std::function<void()>> fns{setter};
        for (int r = 0; r < READERS; ++r) fns.push_back(reader);
        run_all(fns);
        snapshots += snaps.load();
        newer_value += newer.load();
    }
    lt_opt_reset_process();
    printf("ordering (%s): %d rounds x %d steps, %ld snapshots, %ld of them a newer value under an older generation (allowed)\n",
           engine_slot ? "engine slot" : "process default", ROUNDS, STEPS, snapshots, newer_value);
}

// ---- 3 ------------------------------------------------------------------------------------------------------------------------
void check_locality_and_nesting() {
    constexpr int ROUNDS = 200;
    const int id = OPT_GEMM_STAGGER, other = OPT_GEMM_GROUP;
    for (int round = 0; round < ROUNDS; ++round) {
        LtEngineOptions ea, eb;
        lt_opt_set_process(id, 11);
        engine_set(ea, id, 22);
        engine_set(eb, id, 33);
        engine_set(eb, id, 33);  // (generation 2: told apart from ea's 1)
        std::atomic<int> stage{0};
        auto wait_for = [&](int s) { while (stage.load() < s) std::this_thread::yield(); };
        auto thread_a = [&] {
            const int g_outer = lt_opt_generation();
            {
                LtOptScope outer(&ea);
                CHECK(lt_opt(id) == 22 && lt_opt_engine_generation() == 1 && lt_opt_generation() == g_outer, "nesting: outer scope at entry");
                stage.store(1);   // B looks while this scope is open
                wait_for(2);      // B has bumped the process generation and opened a scope of its own
                CHECK(lt_opt(id) == 22 && lt_opt_generation() == g_outer, "locality: thread B's scope or its change reached thread A's scope");
                {
                    LtOptScope inner(&eb);
                    CHECK(lt_opt(id) == 33 && lt_opt_engine_generation() == 2, "nesting: inner scope reads its own engine");
                    CHECK(lt_opt_generation() == g_outer + 1 && lt_opt(other) == 5, "nesting: inner scope reads the process state of its entry");
                    {
                        LtOptScope none(nullptr);
                        CHECK(lt_opt(id) == 11 && lt_opt_engine_generation() == 0, "nesting: a scope without an engine reads process defaults");
                    }
                    CHECK(lt_opt(id) == 33 && lt_opt_engine_generation() == 2, "nesting: inner scope restored");
                }
                CHECK(lt_opt(id) == 22 && lt_opt_engine_generation() == 1 && lt_opt_generation() == g_outer && lt_opt(other) != 5,
                      "nesting: outer scope restored, generations included");
                stage.store(3);
            }
            CHECK(lt_opt(id) == 11 && lt_opt_engine_generation() == 0 && lt_opt_generation() == g_outer + 1 && lt_opt(other) == 5,
                  "nesting: process defaults after the last scope closed");
        };
        auto thread_b = [&] {
            wait_for(1);
            CHECK(lt_opt(id) == 11 && lt_opt_engine_generation() == 0, "locality: thread A's scope is visible on thread B");
            lt_opt_set_process(other, 5);
            {
                LtOptScope mine(&eb);
                CHECK(lt_opt(id) == 33 && lt_opt_engine_generation() == 2, "locality: thread B's own scope");
                stage.store(2);
                wait_for(3);
                CHECK(lt_opt(id) == 33, "locality: thread A's nesting reached thread B's scope");
            }
            CHECK(lt_opt(id) == 11 && lt_opt_engine_generation() == 0, "locality: thread B after its scope");
        };
        run_all({thread_a, thread_b});
        lt_opt_reset_process();
    }
    printf("locality and nesting: %d rounds\n", ROUNDS);
}

// ---- 4 ------------------------------------------------------------------------------------------------------------------------
// engine values 100 .. 199, process values 0 .. 99: a snapshot's value names its source, and LT_OPT_INHERIT itself is in neither set
void check_override_resolution() {
    constexpr int READERS = 2, SCOPES = 20000;
    LtEngineOptions eng;
    const int id = OPT_GEMM_STAGGER;
    lt_opt_set_process(id, 0);
    std::atomic<int> readers_left{READERS};
    std::atomic<long> from_engine{0}, from_process{0};
    auto engine_setter = [&] {
        Lcg r{7};
        while (readers_left.load() > 0) {
            engine_set(eng, id, 100 + (int)(r.next() % 100));
            engine_set(eng, id, LT_OPT_INHERIT);
        }
    };
    auto process_setter = [&] {
        Lcg r{9};
        while (readers_left.load() > 0) lt_opt_set_process(id, (int)(r.next() % 100));
    };
    auto reader = [&] {
        for (int k = 0; k < SCOPES; ++k) {
            LtOptScope scope(&eng);
            const int v = lt_opt(id);
            CHECK(v >= 0 && v <= 199, "override: a snapshot holds %d - neither an engine value (100..199) nor a process default (0..99)%s", v,
                  v == LT_OPT_INHERIT ? ": LT_OPT_INHERIT itself" : "");
            (v >= 100 ? from_engine : from_process).fetch_add(1);
            if (k % 16 == 0) std::this_thread::yield();
        }
        readers_left.fetch_sub(1);
    };
    run_all({engine_setter, process_setter, reader, reader});
    lt_opt_reset_process();
    printf("override resolution: %d snapshots, %ld from the engine slot, %ld from the process default\n", READERS * SCOPES, from_engine.load(),
           from_process.load());
}
}  // namespace

int main() {
    check_constancy();
    check_ordering(false);
    check_ordering(true);
    check_locality_and_nesting();
    check_override_resolution();
    const long f = g_failures.load();
    if (f) {
        fprintf(stderr, "options_threads: %ld check(s) failed\n", f);
        return 1;
    }
    printf("options_threads: ok\n");
    return 0;
}
