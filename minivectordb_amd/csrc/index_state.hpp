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

    // The same windows over a MEAN (the front form of the int8 prefilter: the rows its stage 0 could not reject).  *sum is a
    // running total and *count the device's calls it covers — the device mirrors the pair together, so their quotient does
    // not depend on how far the words lag.  When the mean per call over a window of kSingleWindow host calls exceeds
    // `limit`, the next kSingleSuspend calls are suspended.  A window in which the device counted no call decides nothing.
    std::atomic<unsigned long long> window_sum{0};
    bool suspended_mean(const volatile unsigned long long* sum, const volatile unsigned int* count, double limit) {
        if (suspend_left.load(std::memory_order_relaxed) > 0) {
            suspend_left.fetch_sub(1, std::memory_order_relaxed);
            return true;
        }
        const unsigned int now = calls.fetch_add(1, std::memory_order_relaxed) + 1;
        if (now - window_calls.load(std::memory_order_relaxed) >= (unsigned int)kSingleWindow && sum && count) {
            const unsigned long long s = *sum;
            const unsigned int c = *count;
            const unsigned int dc = c - window_fail.load(std::memory_order_relaxed);
            const unsigned long long ds = s - window_sum.load(std::memory_order_relaxed);
            // (dc, ds as signed: words of two streams may land out of order)
            if ((int)dc > 0 && (long long)ds > 0 && (double)ds > limit * (double)dc) {
                suspend_left.store(kSingleSuspend, std::memory_order_relaxed);
                suspensions.fetch_add(1, std::memory_order_relaxed);
            }
            window_calls.store(now, std::memory_order_relaxed);
            window_fail.store(c, std::memory_order_relaxed);
            window_sum.store(s, std::memory_order_relaxed);
        }
        return false;
    }
    void restart_mean(const volatile unsigned long long* sum, const volatile unsigned int* count) {
        suspend_left.store(0);
        window_calls.store(calls.load());
        if (sum && count) {
            window_sum.store(*sum);
            window_fail.store(*count);
        }
    }
};

}  // namespace mvdb
