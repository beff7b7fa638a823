// Host-only check of the suspension window of the single-query routes (minivectordb_amd/csrc/index_state.hpp: RouteWindow)
// for two sanitizer builds: the window arithmetic, and eight threads deciding at once against a refusal count that moves.
//   c++ -std=c++17 -O1 -g -pthread -I../../minivectordb_amd/csrc -fsanitize=address,undefined -o route_window_asan route_window_host.cpp && ./route_window_asan
//   c++ -std=c++17 -O1 -g -pthread -I../../minivectordb_amd/csrc -fsanitize=thread -o route_window_tsan route_window_host.cpp && ./route_window_tsan
// Runs on the CPU; it never touches a device.  In the library the count is a host-mapped word that the DEVICE writes: here a
// child process writes it through shared memory, so that — as there — no thread of this process ever does.
#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <thread>
#include <vector>

#include "index_state.hpp"

using namespace mvdb;

static int fails = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);    \
            ++fails;                                              \
        }                                                         \
    } while (0)

// n calls: how many were suspended
static int run(RouteWindow& w, const volatile unsigned int* word, int n) {
    int suspended = 0;
    for (int i = 0; i < n; ++i) suspended += w.suspended(word);
    return suspended;
}

static void windows() {
    {   // half of a window refused: the next kSingleSuspend calls are suspended, exactly, then the route probes again
        RouteWindow w;
        volatile unsigned int word = 0;
        CHECK(run(w, &word, kSingleWindow - 1) == 0);
        word = kSingleWindow / 2;                       // 16 counted refusals by the time the window closes
        CHECK(!w.suspended(&word));                     // (the call that closes the window is itself served)
        CHECK(w.suspend_left.load() == kSingleSuspend && w.suspensions.load() == 1);
        CHECK(run(w, &word, kSingleSuspend) == kSingleSuspend);
        CHECK(w.calls.load() == (unsigned int)kSingleWindow);   // (suspended calls are not counted into a window)
        CHECK(!w.suspended(&word));                     // call 513 probes
        CHECK(w.calls.load() == (unsigned int)kSingleWindow + 1 && w.suspensions.load() == 1 && w.suspend_left.load() == 0);
        // restart() in the middle of a suspension: none is pending, and the window starts at the current counts
        word += kSingleWindow;
        CHECK(run(w, &word, kSingleWindow - 1) == 0);
        CHECK(w.suspensions.load() == 2 && w.suspend_left.load() == kSingleSuspend);
        CHECK(run(w, &word, 100) == 100);
        w.restart(&word);
        CHECK(w.suspend_left.load() == 0 && w.window_calls.load() == w.calls.load() && w.window_fail.load() == word);
        word += kSingleWindow / 2 - 1;                  // 15 refusals since the restart: its first window does not suspend ...
        CHECK(run(w, &word, kSingleWindow) == 0 && w.suspensions.load() == 2);
        word += kSingleWindow / 2;                      // ... 16 in the one after do
        CHECK(run(w, &word, kSingleWindow) == 0 && w.suspensions.load() == 3);
        CHECK(w.suspended(&word));
    }
    {   // one refusal short of half: never suspended, window after window
        RouteWindow w;
        volatile unsigned int word = 0;
        for (int win = 0; win < 8; ++win) {
            CHECK(run(w, &word, kSingleWindow - 1) == 0);
            word += kSingleWindow / 2 - 1;
            CHECK(!w.suspended(&word));
        }
        CHECK(w.suspensions.load() == 0 && w.suspend_left.load() == 0 && w.window_calls.load() == 8u * kSingleWindow);
    }
    {   // no mirror yet: never suspended, no window is ever closed
        RouteWindow w;
        CHECK(run(w, nullptr, 4 * kSingleSuspend) == 0);
        CHECK(w.suspensions.load() == 0 && w.window_calls.load() == 0 && w.calls.load() == 4u * kSingleSuspend);
        w.restart(nullptr);
        CHECK(w.window_calls.load() == 4u * kSingleSuspend && w.window_fail.load() == 0);
    }
}

// The window over a mean (the front form of the int8 prefilter: suspended_mean): *sum a running total, *count the device's
// calls it covers, limit the mean per call above which the next kSingleSuspend calls are suspended.
static int run_mean(RouteWindow& w, const volatile unsigned long long* sum, const volatile unsigned int* count, double limit, int n) {
    int suspended = 0;
    for (int i = 0; i < n; ++i) suspended += w.suspended_mean(sum, count, limit);
    return suspended;
}

static void means() {
    const double limit = 1000.0;
    {   // a window whose mean is above the limit suspends, exactly kSingleSuspend calls; at the limit it does not
        RouteWindow w;
        volatile unsigned long long sum = 0;
        volatile unsigned int count = 0;
        CHECK(run_mean(w, &sum, &count, limit, kSingleWindow - 1) == 0);
        count = kSingleWindow - 1;                      // (the device lags by the call in flight)
        sum = 1000ull * (kSingleWindow - 1);            // the mean is the limit: served on
        CHECK(!w.suspended_mean(&sum, &count, limit) && w.suspensions.load() == 0);
        CHECK(w.window_sum.load() == sum && w.window_fail.load() == count);
        CHECK(run_mean(w, &sum, &count, limit, kSingleWindow - 1) == 0);
        count += kSingleWindow;
        sum += 1000ull * kSingleWindow + 1;             // one row above
        CHECK(!w.suspended_mean(&sum, &count, limit));
        CHECK(w.suspend_left.load() == kSingleSuspend && w.suspensions.load() == 1);
        CHECK(run_mean(w, &sum, &count, limit, kSingleSuspend) == kSingleSuspend);
        CHECK(!w.suspended_mean(&sum, &count, limit) && w.suspend_left.load() == 0);
        // a window in which the device counted no call decides nothing, whatever the sum reads
        sum += 1ull << 40;
        CHECK(run_mean(w, &sum, &count, limit, 2 * kSingleWindow) == 0 && w.suspensions.load() == 1);
        // words that land out of order (the count or the sum steps back): nothing is decided, the window moves on
        count += 10;
        sum -= 5;
        CHECK(run_mean(w, &sum, &count, limit, kSingleWindow) == 0 && w.suspensions.load() == 1);
        // restart_mean in the middle of a suspension
        count += kSingleWindow;
        sum += 2000ull * kSingleWindow;
        CHECK(run_mean(w, &sum, &count, limit, kSingleWindow - 1) == 0 && w.suspensions.load() == 2);   // (the 31 calls to the window's end)
        CHECK(run_mean(w, &sum, &count, limit, 100) == 100);
        w.restart_mean(&sum, &count);
        CHECK(w.suspend_left.load() == 0 && w.window_calls.load() == w.calls.load() && w.window_sum.load() == sum && w.window_fail.load() == count);
        CHECK(run_mean(w, &sum, &count, limit, kSingleWindow) == 0 && w.suspensions.load() == 2);
    }
    {   // no mirror yet: never suspended
        RouteWindow w;
        CHECK(run_mean(w, nullptr, nullptr, limit, 4 * kSingleSuspend) == 0 && w.suspensions.load() == 0 && w.window_calls.load() == 0);
        w.restart_mean(nullptr, nullptr);
        CHECK(w.window_calls.load() == 4u * kSingleSuspend);
    }
}

static void threads() {
    constexpr int kThreads = 8, kCalls = 100000;
    // [0] the refusal count, [1] the stop flag: written by the child and by the main thread respectively
    volatile unsigned int* shared =
        (volatile unsigned int*)mmap(nullptr, 4096, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (shared == MAP_FAILED) {
        CHECK(!"mmap");
        return;
    }
    shared[0] = shared[1] = shared[2] = shared[3] = 0;
    const pid_t parent = getpid();
    const pid_t child = fork();
    if (child == 0) {   // the "device": refusals arrive while the threads decide, in bursts with quiet stretches between
        while (!shared[1] && getppid() == parent) {
            for (int burst = 0; burst < 256; ++burst) {
                shared[0] = shared[0] + 1;
                *(volatile unsigned long long*)(shared + 2) = (unsigned long long)shared[0] * 3;   // (a mean of 3 per call)
            }
            for (volatile int quiet = 0; quiet < 2000; quiet = quiet + 1) {}
        }
        _exit(0);
    }
    CHECK(child > 0);
    RouteWindow w;
    int lowest[kThreads], suspended[kThreads];
    std::vector<std::thread> pool;
    for (int t = 0; t < kThreads; ++t)
        pool.emplace_back([&, t] {
            int lo = 0, sus = 0;
            for (int i = 0; i < kCalls; ++i) {
                sus += w.suspended(shared);
                lo = std::min(lo, w.suspend_left.load(std::memory_order_relaxed));
            }
            lowest[t] = lo;
            suspended[t] = sus;
        });
    for (auto& th : pool) th.join();
    // the same eight threads over the mean's window: the child's word as the count of calls, its square-ish sum beside it
    {
        RouteWindow wm;
        volatile unsigned long long* sum = (volatile unsigned long long*)(shared + 2);   // (8-byte aligned: the page's offset 8)
        std::vector<std::thread> pool2;
        std::atomic<long long> sus2{0};
        for (int t = 0; t < kThreads; ++t)
            pool2.emplace_back([&] {
                long long sus = 0;
                for (int i = 0; i < kCalls; ++i) sus += wm.suspended_mean(sum, shared, 0.5);
                sus2 += sus;
            });
        for (auto& th : pool2) th.join();
        CHECK(wm.calls.load() + (unsigned long long)sus2.load() == (unsigned long long)kThreads * kCalls);
        CHECK(wm.suspensions.load() > 0);
    }
    shared[1] = 1;
    int status = -1;
    if (child > 0) CHECK(waitpid(child, &status, 0) == child && WIFEXITED(status) && WEXITSTATUS(status) == 0);
    long long total = 0;
    int lo = 0;
    for (int t = 0; t < kThreads; ++t) {
        total += suspended[t];
        lo = std::min(lo, lowest[t]);
    }
    // every thread that saw a positive count may take one: the count never falls below minus the number of threads
    CHECK(lo >= -kThreads);
    CHECK(shared[0] > 0 && w.suspensions.load() > 0 && total > 0);
    CHECK(w.calls.load() + (unsigned long long)total == (unsigned long long)kThreads * kCalls);
    std::printf("threads: %d x %d calls, %llu refusals counted, %llu suspensions, %lld calls suspended, lowest suspend_left %d\n", kThreads,
                kCalls, (unsigned long long)shared[0], w.suspensions.load(), total, lo);
    munmap((void*)shared, 4096);
}

int main() {
    windows();
    means();
    threads();
    std::printf(fails ? "route_window_host: %d check(s) FAILED\n" : "route_window_host: ok\n", fails);
    return fails ? 1 : 0;
}
