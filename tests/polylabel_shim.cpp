// Host build of osm_renderer_amd/host/osmt_labelable.hpp (the scalar statement of the label-position function) for the
// CPU-side tests and the CPU side of tools/bench_polylabel.py, plus sizeof / offsetof probes of the label-anchor ABI.
// Built with OSMT_LABELABLE_DEBUG: the mirror counts every NaN that reaches the distance minimum or a queue key.
#define OSMT_LABELABLE_DEBUG 1
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>

#include "../include/osmtile.h"
#include "../osm_renderer_amd/host/osmt_labelable.hpp"

extern "C" {
// out[i] = get_label_position of request i (capped: with the device's TOO_LARGE rule); peak / pops (optional): the queue
// peak and the pop count of each run.  Returns the number of NaNs seen where none may be (0).
uint64_t shim_polylabel_batch(const osmt_label_request* req, size_t n_req, const osmt_ring* rings, const double* pts, int capped,
                              int threads, osmt_label_position* out, uint64_t* peak, uint64_t* pops) {
    std::atomic<uint64_t> nans{0};
    std::atomic<size_t> next{0};
    auto work = [&] {
        std::vector<const double*> p;
        std::vector<uint32_t> n;
        uint64_t bad = 0;
        for (;;) {
            const size_t lo = next.fetch_add(64);
            if (lo >= n_req) break;
            for (size_t i = lo; i < n_req && i < lo + 64; ++i) {
                p.resize(req[i].n_rings);
                n.resize(req[i].n_rings);
                for (uint32_t k = 0; k < req[i].n_rings; ++k) {
                    p[k] = pts + 2 * (size_t)rings[req[i].ring_off + k].first_pt;
                    n[k] = rings[req[i].ring_off + k].n_pts;
                }
                osmt::LabelSearchStats st;
                const osmt::LabelPosition r = osmt::get_label_position(p.data(), n.data(), req[i].n_rings, req[i].scale, capped != 0, &st);
                out[i].x = r.x;
                out[i].y = r.y;
                out[i].status = r.status;
                out[i]._pad = 0;
                if (peak) peak[i] = st.queue_peak;
                if (pops) pops[i] = st.pops;
                bad += st.nan_to_min;
            }
        }
        nans += bad;
    };
    if (threads <= 1) {
        work();
    } else {
        std::vector<std::thread> th;
        for (int t = 0; t < threads; ++t) th.emplace_back(work);
        for (auto& t : th) t.join();
    }
    return nans.load();
}

size_t shim_polylabel_sizeof(int what) {
    switch (what) {
        case 0: return sizeof(osmt_label_request);
        case 1: return sizeof(osmt_label_position);
        case 2: return sizeof(osmt_label_request_batch);
        case 10: return offsetof(osmt_label_request, scale);
        case 11: return offsetof(osmt_label_position, status);
        case 12: return offsetof(osmt_label_request_batch, points);
        case 13: return offsetof(osmt_label_request_batch, n_pts);
        default: return 0;
    }
}
}
