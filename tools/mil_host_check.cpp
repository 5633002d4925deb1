// Host-side check of the argument validation of the MIL exports (csrc/mil.hip): wssdl_mil_pool_forward,
// wssdl_mil_pool_backward, and what wssdl_mil_select / wssdl_mil_loss_forward do with the selectors 3 and 4.  Every
// rejected call must return WSSDL_ERR_INVALID_ARGUMENT before anything is launched, so this runs without a GPU, under
// the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       wssdl_bus_amd/csrc/mil.hip wssdl_bus_amd/csrc/api_common.hip tools/mil_host_check.cpp \
//       -o mil_host_check && ./mil_host_check
//
// The pointers that stand for device memory are never dereferenced on the host: they point at small host arrays so
// that a validation that did read them would be seen by the sanitizer rather than fault.  class_weights_host IS host
// memory and is read.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/wssdl_bus_hip.h"

int main() {
    const int R = 6, K = 3, NB = 2;
    std::vector<float> logits(R * K, 0.f), col(R, 0.f), cw(8, 0.5f), loss(1, 0.f), bag_logits(NB * K, 0.f), bag_loss(NB, 0.f),
        gl(1, 1.f), grad(R * K, 0.f);
    std::vector<int32_t> labels(NB, 1), rows(NB, 0), counts(NB, 0);
    int bad = 0, n = 0;
    auto expect = [&](const char *what, bool ok) {
        ++n;
        if (!ok) {
            ++bad;
            std::printf("FAIL %s\n", what);
        }
    };
    const int E = WSSDL_ERR_INVALID_ARGUMENT;
    struct F {                                                       // the arguments of a valid forward call
        const float *logits; int R, K; const float *col; int stride; const int32_t *labels; int nb, s1, s2;
        const float *cw; float *loss; int32_t *rows, *counts; float *bag_logits, *bag_loss;
    };
    const F f0 = {logits.data(), R, K, col.data(), 1, labels.data(), NB, 3, 4, cw.data(), loss.data(), rows.data(),
                  counts.data(), bag_logits.data(), bag_loss.data()};
    auto fwd = [&](const F &a) {
        return wssdl_mil_pool_forward(a.logits, a.R, a.K, a.col, a.stride, 0.f, a.labels, a.nb, a.s1, a.s2, a.cw, 1.f, a.loss,
                                      a.rows, a.counts, a.bag_logits, a.bag_loss, nullptr);
    };
    F a = f0;
    a.logits = nullptr;      expect("forward: null logits", fwd(a) == E);            a = f0;
    a.col = nullptr;         expect("forward: null bag column", fwd(a) == E);        a = f0;
    a.labels = nullptr;      expect("forward: null bag labels", fwd(a) == E);        a = f0;
    a.cw = nullptr;          expect("forward: null class weights", fwd(a) == E);     a = f0;
    a.loss = nullptr;        expect("forward: null loss", fwd(a) == E);              a = f0;
    a.rows = nullptr;        expect("forward: null row_out", fwd(a) == E);           a = f0;
    a.counts = nullptr;      expect("forward: null bag_count", fwd(a) == E);         a = f0;
    a.bag_logits = nullptr;  expect("forward: null bag_logits", fwd(a) == E);        a = f0;
    a.bag_loss = nullptr;    expect("forward: null bag_loss", fwd(a) == E);          a = f0;
    a.K = 2;                 expect("forward: K = 2", fwd(a) == E);                  a = f0;
    a.K = 9;                 expect("forward: K = 9", fwd(a) == E);                  a = f0;
    a.K = -1;                expect("forward: K = -1", fwd(a) == E);                 a = f0;
    a.R = -1;                expect("forward: R = -1", fwd(a) == E);                 a = f0;
    a.nb = 0;                expect("forward: n_bags = 0", fwd(a) == E);             a = f0;
    a.nb = -3;               expect("forward: n_bags = -3", fwd(a) == E);            a = f0;
    a.stride = 0;            expect("forward: bag_stride = 0", fwd(a) == E);         a = f0;
    a.stride = -5;           expect("forward: bag_stride = -5", fwd(a) == E);        a = f0;
    a.s1 = 5;                expect("forward: selector_label1 = 5", fwd(a) == E);    a = f0;
    a.s1 = -1;               expect("forward: selector_label1 = -1", fwd(a) == E);   a = f0;
    a.s2 = 5;                expect("forward: selector_other = 5", fwd(a) == E);     a = f0;
    a.s2 = -1;               expect("forward: selector_other = -1", fwd(a) == E);    a = f0;

    struct B {
        const float *logits; int R, K; const float *col; int stride; const int32_t *labels; int nb, s1, s2;
        const int32_t *rows, *counts; const float *bag_logits, *cw, *gl; float *grad;
    };
    const B b0 = {logits.data(), R, K, col.data(), 1, labels.data(), NB, 4, 3, rows.data(), counts.data(), bag_logits.data(),
                  cw.data(), gl.data(), grad.data()};
    auto bwd = [&](const B &x) {
        return wssdl_mil_pool_backward(x.logits, x.R, x.K, x.col, x.stride, 0.f, x.labels, x.nb, x.s1, x.s2, x.rows, x.counts,
                                       x.bag_logits, x.cw, 1.f, x.gl, x.grad, nullptr);
    };
    B b = b0;
    b.logits = nullptr;      expect("backward: null logits", bwd(b) == E);           b = b0;
    b.col = nullptr;         expect("backward: null bag column", bwd(b) == E);       b = b0;
    b.labels = nullptr;      expect("backward: null bag labels", bwd(b) == E);       b = b0;
    b.rows = nullptr;        expect("backward: null rows", bwd(b) == E);             b = b0;
    b.counts = nullptr;      expect("backward: null bag_count", bwd(b) == E);        b = b0;
    b.bag_logits = nullptr;  expect("backward: null bag_logits", bwd(b) == E);       b = b0;
    b.cw = nullptr;          expect("backward: null class weights", bwd(b) == E);    b = b0;
    b.gl = nullptr;          expect("backward: null grad_loss", bwd(b) == E);        b = b0;
    b.grad = nullptr;        expect("backward: null grad_logits", bwd(b) == E);      b = b0;
    b.K = 2;                 expect("backward: K = 2", bwd(b) == E);                 b = b0;
    b.K = 9;                 expect("backward: K = 9", bwd(b) == E);                 b = b0;
    b.R = -1;                expect("backward: R = -1", bwd(b) == E);                b = b0;
    b.nb = 0;                expect("backward: n_bags = 0", bwd(b) == E);            b = b0;
    b.stride = 0;            expect("backward: bag_stride = 0", bwd(b) == E);        b = b0;
    b.s1 = 5;                expect("backward: selector_label1 = 5", bwd(b) == E);   b = b0;
    b.s1 = -1;               expect("backward: selector_label1 = -1", bwd(b) == E);  b = b0;
    b.s2 = 5;                expect("backward: selector_other = 5", bwd(b) == E);    b = b0;
    b.s2 = -2;               expect("backward: selector_other = -2", bwd(b) == E);   b = b0;
    b.R = 0;                 expect("backward: nothing to do with R = 0", bwd(b) == WSSDL_OK);   b = b0;

    // the older exports and the two new selectors
    auto sel = [&](int s1, int s2) {
        return wssdl_mil_select(logits.data(), R, K, col.data(), 1, 0.f, labels.data(), NB, s1, s2, rows.data(), nullptr, nullptr);
    };
    expect("select: selector 5", sel(5, 0) == E);
    expect("select: selector -1", sel(0, -1) == E);
    expect("select: n_bags = 0 is nothing to do", wssdl_mil_select(logits.data(), R, K, col.data(), 1, 0.f, labels.data(), 0, 3, 4,
                                                                   rows.data(), nullptr, nullptr) == WSSDL_OK);
    auto old_fwd = [&](int s1, int s2, int stride) {
        return wssdl_mil_loss_forward(logits.data(), R, K, col.data(), stride, 0.f, labels.data(), NB, s1, s2, cw.data(), 1.f,
                                      loss.data(), rows.data(), bag_loss.data(), nullptr);
    };
    expect("loss_forward: mean-ben for bags labelled 1", old_fwd(4, 0, 1) == E);
    expect("loss_forward: mean-ben for the others", old_fwd(0, 4, 1) == E);
    expect("loss_forward: selector 5", old_fwd(5, 0, 1) == E);
    expect("loss_forward: bag_stride = 0", old_fwd(0, 0, 0) == E);
    std::printf("%d checks, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
