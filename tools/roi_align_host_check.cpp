// Host-side check of the argument validation of the RoIAlign exports (csrc/roi_align.hip): wssdl_roi_align_tables,
// wssdl_roi_align_forward, wssdl_roi_align_backward_prepare, wssdl_roi_align_backward and the two size queries.  Every
// rejected call must return WSSDL_ERR_INVALID_ARGUMENT with wssdl_last_error set before anything is launched, and R = 0
// is a valid call that launches nothing, so this runs without a GPU, under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       wssdl_bus_amd/csrc/roi_align.hip wssdl_bus_amd/csrc/api_common.hip tools/roi_align_host_check.cpp \
//       -o roi_align_host_check && ./roi_align_host_check
//
// The pointers that stand for device memory are never dereferenced on the host: they point at small host arrays so
// that a validation that did read them would be seen by the sanitizer rather than fault.  (The zero fill of the
// backward's R = 0 call is enqueued work and is left to the GPU tests.)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/wssdl_bus_hip.h"

int main() {
    int bad = 0, n = 0;
    auto expect = [&](const char *what, bool ok) {
        ++n;
        if (!ok) {
            ++bad;
            std::printf("FAIL %s\n", what);
        }
    };
    struct A {                                                      // the arguments of a valid call of each export
        int R, N, H, W, C, PH, PW, S, aligned;
        const float *rois, *bottom, *top_diff;
        float *top, *bottom_diff;
        void *tables, *ws;
        size_t nt, nws;
    };
    std::vector<float> rois(5 * 5, 0.f), small(16, 0.f);
    A a0 = {5, 2, 6, 9, 8, 7, 7, 2, 1, rois.data(), small.data(), small.data(), small.data(), small.data(), nullptr, nullptr, 0, 0};
    a0.nt = wssdl_roi_align_tables_bytes(a0.R, a0.PH, a0.PW, a0.S);
    a0.nws = wssdl_roi_align_backward_workspace_bytes(a0.R, a0.N, a0.H, a0.W);
    expect("tables_bytes: 5 RoIs, 7 x 7, S = 2", a0.nt == 5u * (4 * 7 * 2 + 4 * 7 * 2 + 5) * 4u);
    expect("tables_bytes: S = 0", wssdl_roi_align_tables_bytes(5, 7, 7, 0) == 0);
    expect("tables_bytes: pooled_h = 17", wssdl_roi_align_tables_bytes(5, 17, 7, 2) == 0);
    expect("tables_bytes: R = -1", wssdl_roi_align_tables_bytes(-1, 7, 7, 2) == 0);
    expect("workspace_bytes: valid", a0.nws > 0);
    expect("workspace_bytes: N = 0", wssdl_roi_align_backward_workspace_bytes(5, 0, 6, 9) == 0);
    expect("workspace_bytes: H = 0", wssdl_roi_align_backward_workspace_bytes(5, 2, 0, 9) == 0);
    std::vector<char> tables(a0.nt, 0), ws(a0.nws, 0);
    a0.tables = tables.data();
    a0.ws = ws.data();

    auto call = [&](int which, const A &a) {
        switch (which) {
        case 0:
            return wssdl_roi_align_tables(a.rois, a.R, a.N, a.H, a.W, a.PH, a.PW, 0.0625f, a.S, a.aligned, a.tables, a.nt, nullptr);
        case 1:
            return wssdl_roi_align_forward(a.bottom, a.N, a.H, a.W, a.C, a.R, a.PH, a.PW, a.S, a.tables, a.nt, a.top, nullptr);
        case 2:
            return wssdl_roi_align_backward_prepare(a.R, a.N, a.H, a.W, a.PH, a.PW, a.S, a.tables, a.nt, a.ws, a.nws, nullptr);
        default:
            return wssdl_roi_align_backward(a.top_diff, a.R, a.N, a.H, a.W, a.C, a.PH, a.PW, a.S, a.tables, a.nt, a.ws, a.nws,
                                            a.bottom_diff, nullptr);
        }
    };
    const char *names[4] = {"tables", "forward", "backward_prepare", "backward"};
    char what[128];
    auto refused = [&](int which, const char *change, const A &a) {
        std::snprintf(what, sizeof what, "%s: %s", names[which], change);
        expect(what, call(which, a) == WSSDL_ERR_INVALID_ARGUMENT && std::strlen(wssdl_last_error()) > 0);
    };
    for (int which = 0; which < 4; ++which) {
        A a = a0;
        a.S = 0;            refused(which, "sampling = 0", a);          a = a0;
        a.S = 5;            refused(which, "sampling = 5", a);          a = a0;
        a.S = -2;           refused(which, "sampling = -2", a);         a = a0;
        a.N = 0;            refused(which, "N = 0", a);                 a = a0;
        a.H = 0;            refused(which, "H = 0", a);                 a = a0;
        a.W = -1;           refused(which, "W = -1", a);                a = a0;
        a.PH = 0;           refused(which, "pooled_h = 0", a);          a = a0;
        a.PH = 17;          refused(which, "pooled_h = 17", a);         a = a0;
        a.PW = 0;           refused(which, "pooled_w = 0", a);          a = a0;
        a.PW = 17;          refused(which, "pooled_w = 17", a);         a = a0;
        a.R = -1;           refused(which, "R = -1", a);                a = a0;
        a.tables = nullptr; refused(which, "null tables", a);           a = a0;
        a.nt -= 4;          refused(which, "tables 4 bytes short", a);  a = a0;
        if (which == 0) {
            a.rois = nullptr;   refused(which, "null rois", a);         a = a0;
            a.aligned = 2;      refused(which, "aligned = 2", a);       a = a0;
        }
        if (which == 1) {
            a.C = 0;            refused(which, "C = 0", a);             a = a0;
            a.bottom = nullptr; refused(which, "null bottom", a);       a = a0;
            a.top = nullptr;    refused(which, "null top", a);          a = a0;
        }
        if (which >= 2) {
            a.ws = nullptr;     refused(which, "null workspace", a);            a = a0;
            a.nws -= 1;         refused(which, "workspace one byte short", a);  a = a0;
        }
        if (which == 3) {
            a.C = -4;                refused(which, "C = -4", a);               a = a0;
            a.top_diff = nullptr;    refused(which, "null top_diff", a);        a = a0;
            a.bottom_diff = nullptr; refused(which, "null bottom_diff", a);     a = a0;
        }
        if (which < 3) {            // R = 0: nothing to do, nothing launched, and the last error is cleared
            a.R = 0;
            a.rois = a.bottom = nullptr;
            a.top = nullptr;
            a.tables = a.ws = nullptr;
            a.nt = a.nws = 0;
            std::snprintf(what, sizeof what, "%s: R = 0 is nothing to do", names[which]);
            expect(what, call(which, a) == WSSDL_OK && std::strlen(wssdl_last_error()) == 0);
        }
    }
    std::printf("%d checks, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
