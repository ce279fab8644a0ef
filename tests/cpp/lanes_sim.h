// lanes_sim.h -- a simulated lane group for the stand-alone host tests: what seqlib_amd/csrc/dev_lanes.h's lanes_group<G> is on the GPU, with a thread per lane.
// The lanes of a GPU group run in step; here every collective goes through a barrier.  A body that takes `lane` of `nlanes` and a lane policy (cov_record,
// pile_record) runs under it unchanged: lanes_run(nlanes, body) calls body(lane, W) on nlanes threads.  Build with -pthread.
#pragma once
#include <pthread.h>
#include <cstdint>
#include <thread>
#include <vector>

// what the lanes of a simulated group share: two sets of slots taken in turn, so that one barrier a collective is enough (a lane that writes set k again has
// passed the barrier of the collective on the other set, behind which every lane has read set k)
struct Group {
    pthread_barrier_t bar;
    uint64_t slot[2][64];
    uint32_t nlanes;
};
struct GroupLane {
    Group *g; uint32_t lane; mutable uint32_t turn;
    const uint64_t *exchange(uint64_t v) const
    {
        uint64_t *s = g->slot[turn & 1u];
        ++turn;
        s[lane] = v;
        pthread_barrier_wait(&g->bar);
        return s;
    }
    uint64_t scan(uint64_t v, uint64_t *total) const
    {
        const uint64_t *s = exchange(v);
        uint64_t before = 0, all = 0;
        for (uint32_t i = 0; i < g->nlanes; ++i) { if (i < lane) before += s[i]; all += s[i]; }
        *total = all;
        return before;
    }
    uint64_t bcast(uint64_t v, uint32_t j) const { return exchange(v)[j]; }
    uint64_t sum(uint64_t v) const { uint64_t total; (void)scan(v, &total); return total; }
    uint64_t min(uint64_t v) const { const uint64_t *s = exchange(v); uint64_t m = s[0]; for (uint32_t i = 1; i < g->nlanes; ++i) m = s[i] < m ? s[i] : m; return m; }
    uint64_t max(uint64_t v) const { const uint64_t *s = exchange(v); uint64_t m = s[0]; for (uint32_t i = 1; i < g->nlanes; ++i) m = s[i] > m ? s[i] : m; return m; }
};

// body(lane, W) on nlanes (at most 64) threads that share one group
template <class Body> static void lanes_run(uint32_t nlanes, Body body)
{
    Group g;
    g.nlanes = nlanes;
    pthread_barrier_init(&g.bar, nullptr, nlanes);
    std::vector<std::thread> th;
    for (uint32_t l = 0; l < nlanes; ++l) th.emplace_back([&, l]() { GroupLane W = {&g, l, 0u}; body(l, W); });
    for (auto &t : th) t.join();
    pthread_barrier_destroy(&g.bar);
}
