// index_state.hpp — host-only state of the flat index (plain C++, no HIP): what can be compiled and tested without a device.
#pragma once
#include <atomic>

namespace mvdb {

// A single-query route that costs MORE than the exact scan when the device refuses its answer (the shadow route: the
// nomination pass, then the exact scan anyway — 0.59 against 0.31 ms per query on a clustered 1M x 512 corpus, BENCH
// certified_passes_on_unfriendly_data; the int8 route: its fallback).  The device keeps a running count of refusals and
// mirrors it into a host-mapped word; the routing looks at windows of kSingleWindow calls and, when half of a window was
// refused, sends the next kSingleSuspend calls straight to the exact scan before it probes again.  No synchronisation: the
// word lags by the calls in flight, which a heuristic can afford.  `fails` is that word; NULL (no mirror yet): never suspends.
constexpr int kSingleWindow = 32, kSingleSuspend = 512;
struct RouteWindow {
    std::atomic<unsigned int> calls{0}, window_calls{0}, window_fail{0};
    std::atomic<int> suspend_left{0};
    std::atomic<unsigned long long> suspensions{0};

    // One decision per call the route would serve: true = suspended, the exact scan answers.
    bool suspended(const volatile unsigned int* fails) {
        if (suspend_left.load(std::memory_order_relaxed) > 0) {
            suspend_left.fetch_sub(1, std::memory_order_relaxed);
            return true;
        }
        const unsigned int now = calls.fetch_add(1, std::memory_order_relaxed) + 1;
        if (now - window_calls.load(std::memory_order_relaxed) >= (unsigned int)kSingleWindow && fails) {
            const unsigned int f = *fails;
            if ((f - window_fail.load(std::memory_order_relaxed)) * 2 >= (unsigned int)kSingleWindow) {
                suspend_left.store(kSingleSuspend, std::memory_order_relaxed);
                suspensions.fetch_add(1, std::memory_order_relaxed);
            }
            window_calls.store(now, std::memory_order_relaxed);
            window_fail.store(f, std::memory_order_relaxed);
        }
        return false;
    }
    // A fresh start (the route's option was set; the caller holds the index exclusively): the route probes again from its
    // next call, in a window that starts at the current counts.
    void restart(const volatile unsigned int* fails) {
        suspend_left.store(0);
        window_calls.store(calls.load());
        if (fails) window_fail.store(*fails);
    }
};

}  // namespace mvdb
