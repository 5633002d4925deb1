// Host-side check of wsplumb_optim_step's argument validation (csrc/plumbing/optim.hip): every rejected call must
// return 1 before any launch, so this runs without a GPU, under the host sanitizers:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       wssdl_bus_amd/csrc/plumbing/optim.hip tools/optim_host_check.cpp -o optim_host_check && ./optim_host_check
#include <cstdio>

extern "C" int wsplumb_optim_chunk();
extern "C" int wsplumb_optim_step(int kind, const void *tab, int n_chunks, const void *params, const void *grads,
                                  int n_params, float *s0, float *s1, float *s2, float lr, float alpha_t, float eps,
                                  float mu, float b1, float b2, void *stream);

int main() {
    long long tab[4] = {0, 0, 1, 0}, addr[1] = {0};
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int bad = 0, n = 0;
    auto expect1 = [&](const char *what, int rc) {
        ++n;
        if (rc != 1) {
            ++bad;
            std::printf("FAIL %s: rc %d\n", what, rc);
        }
    };
#define STEP(kind, tab, nc, pp, gp, np, s0, s1, s2) \
    wsplumb_optim_step(kind, tab, nc, pp, gp, np, s0, s1, s2, 5e-4f, 5e-4f, 0.1f, 0.9f, 0.9f, 0.999f, nullptr)
    expect1("null table", STEP(0, nullptr, 1, addr, addr, 1, s, s, s));
    expect1("zero chunks", STEP(0, tab, 0, addr, addr, 1, s, s, s));
    expect1("negative chunks", STEP(0, tab, -3, addr, addr, 1, s, s, s));
    expect1("null parameter table", STEP(0, tab, 1, nullptr, addr, 1, s, s, s));
    expect1("null gradient table", STEP(0, tab, 1, addr, nullptr, 1, s, s, s));
    expect1("zero parameters", STEP(0, tab, 1, addr, addr, 0, s, s, s));
    expect1("kind -1", STEP(-1, tab, 1, addr, addr, 1, s, s, s));
    expect1("kind 3", STEP(3, tab, 1, addr, addr, 1, s, s, s));
    expect1("adam without m", STEP(0, tab, 1, addr, addr, 1, nullptr, s, s));
    expect1("adam without v", STEP(0, tab, 1, addr, addr, 1, s, nullptr, s));
    expect1("amsgrad without vhat", STEP(1, tab, 1, addr, addr, 1, s, s, nullptr));
    expect1("nesterov without accum", STEP(2, tab, 1, addr, addr, 1, nullptr, nullptr, nullptr));
    if (wsplumb_optim_chunk() != 4096) {
        ++bad;
        std::printf("FAIL chunk %d\n", wsplumb_optim_chunk());
    }
    std::printf("%d rejected calls checked, %d failures\n", n, bad);
    return bad ? 1 : 0;
}
