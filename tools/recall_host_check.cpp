// Host-side check of wssdl_proposal_recall's argument validation (csrc/proposal_recall.hip): every rejected call must
// return WSSDL_ERR_INVALID_ARGUMENT before anything is launched or copied, so this runs without a GPU, under the host
// sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       wssdl_bus_amd/csrc/proposal_recall.hip wssdl_bus_amd/csrc/api_common.hip tools/recall_host_check.cpp \
//       -o recall_host_check && ./recall_host_check
//
// The pointers that stand for device memory are never dereferenced on the host: they point at small host arrays so
// that a validation that did read them would be seen by the sanitizer rather than fault.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/wssdl_bus_hip.h"

int main() {
    const int N = 3, P = 4, G = 5, A = 2, L = 2, T = 3;
    std::vector<float> f32(N * P * 5, 0.f), scale(N, 1.f);
    std::vector<double> f64(N * P * 4, 0.0), gtb(G * 4, 0.0), gta(G, 0.0), rng(A * 2, 0.0), thr(T, 0.5), mov(A * L * G, 0.0);
    std::vector<int32_t> counts(N, 0), lim(L, 0), hits(A * L * T, 0), npos(A * L, 0), flags(A * L, 0), mgt(A * L * G, 0), mbox(A * L * G, 0);
    int32_t off[N + 1] = {0, 2, 2, 5};
    const size_t need = wssdl_proposal_recall_workspace_bytes(N, P, G);
    std::vector<char> ws(need, 0);
    int bad = 0, n = 0;
    auto expect = [&](const char *what, bool ok) {
        ++n;
        if (!ok) {
            ++bad;
            std::printf("FAIL %s\n", what);
        }
    };
    auto call = [&](const float *b32, const float *sc, const double *b64, int stride, const int32_t *cnt, int n_, int p_,
                    const double *gb, const double *ga, const int32_t *o, int g_, const double *r, int a_, const int32_t *l,
                    int l_, const double *t, int t_, int32_t *h, int32_t *np_, int32_t *fl, void *w, size_t wb) {
        return wssdl_proposal_recall(b32, sc, b64, stride, cnt, n_, p_, gb, ga, o, g_, r, a_, l, l_, t, t_, h, np_, fl, mgt.data(),
                                     mbox.data(), mov.data(), w, wb, nullptr);
    };
    const int E = WSSDL_ERR_INVALID_ARGUMENT;
    expect("workspace query", need >= (size_t)G * P * sizeof(double) + (N + 1) * sizeof(int32_t));
    expect("workspace query rejects N < 0", wssdl_proposal_recall_workspace_bytes(-1, P, G) == 0);
    expect("workspace query rejects P < 0", wssdl_proposal_recall_workspace_bytes(N, -1, G) == 0);
    expect("workspace query rejects P too large", wssdl_proposal_recall_workspace_bytes(N, WSSDL_RECALL_MAX_BOXES + 1, G) == 0);
    expect("workspace query rejects G < 0", wssdl_proposal_recall_workspace_bytes(N, P, -1) == 0);
    expect("workspace query of nothing", wssdl_proposal_recall_workspace_bytes(0, 0, 0) > 0);

    expect("neither box form", call(nullptr, nullptr, nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("both box forms", call(f32.data() + 1, nullptr, f64.data(), 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("scale with the f64 form", call(nullptr, scale.data(), f64.data(), 4, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("row stride 3", call(f32.data() + 1, scale.data(), nullptr, 3, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null counts", call(f32.data() + 1, scale.data(), nullptr, 5, nullptr, N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("negative N", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), -1, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("negative P", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, -4, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("P too large", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, WSSDL_RECALL_MAX_BOXES + 1, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("negative Gtot", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, -5, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null gt boxes", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, nullptr, gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null gt areas", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), nullptr, off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null offsets", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), nullptr, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    {
        const int32_t down[N + 1] = {0, 3, 2, 5}, late[N + 1] = {1, 2, 2, 5}, shortfall[N + 1] = {0, 2, 2, 4}, past[N + 1] = {0, 2, 7, 5};
        int32_t many[N + 1] = {0, 0, 0, WSSDL_RECALL_MAX_GT + 1};
        expect("offsets that decrease", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), down, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
        expect("offsets that rise past Gtot and come back", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), past, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
        expect("offsets that do not start at 0", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), late, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
        expect("offsets that do not end at Gtot", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), shortfall, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
        expect("an image with too many gts", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), many, WSSDL_RECALL_MAX_GT + 1, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), (size_t)1 << 40) == E);
    }
    expect("null area ranges", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, nullptr, A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("A = 0", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), 0, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null limits", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, nullptr, L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("L = -1", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), -1, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null thresholds", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, nullptr, T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("T = 0", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), 0, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("cells beyond an int", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), 1 << 20, lim.data(), 1 << 20, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need) == E);
    expect("null hits", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, nullptr, npos.data(), flags.data(), ws.data(), need) == E);
    expect("null num_pos", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), nullptr, flags.data(), ws.data(), need) == E);
    expect("null flags", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), nullptr, ws.data(), need) == E);
    expect("null workspace", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), nullptr, need) == E);
    expect("workspace one byte short", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), need - 1) == E);
    expect("workspace of nothing", call(f32.data() + 1, scale.data(), nullptr, 5, counts.data(), N, P, gtb.data(), gta.data(), off, G, rng.data(), A, lim.data(), L, thr.data(), T, hits.data(), npos.data(), flags.data(), ws.data(), 0) == E);
    std::printf("%d checks, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
