// optim_main.cpp — a stand-alone host program over achelous_amd/csrc/k_optim.h under the CPU emulator, for the host sanitizers (tests/test_optim.py builds it with
// g++ -fsanitize=address,undefined and runs it; no Python involved).  TEST INFRASTRUCTURE ONLY.
// The arenas are heap blocks of EXACTLY the size the layout gives them, so an index one element past an arena is a report.  The shapes are those of
// tests/optim_cases.py Standin: slot tails (1, 3, 255, 257, 1023, 4097), an exact fit (256), multi-chunk tensors, a parameter without a gradient, one that gains its
// gradient at step 2, one in no group, a float buffer of 5.  Four steps of every kind; afterwards padding must be zero everywhere, the inactive and the ungrouped
// parameter untouched, and the step counts what the activity says.  Exit 0 = all held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "k_optim.h"

namespace {
struct Tensor { int n, flag; bool never, late; int first = 0, chunks = 0; };

int fail(const char* what, int kind, long at) {
    std::fprintf(stderr, "optim_main: %s (kind %d, at %ld)\n", what, kind, at);
    return 1;
}

int run(int kind, float mu, int nesterov, bool with_ema) {
    std::vector<Tensor> ts = {{1, 0, false, false},    {256, 0, false, false}, {4097, 0, false, false}, {300, 0, true, false},  {3, 1, false, false}, {257, 1, false, false},
                              {259, 1, false, true},   {255, 2, false, false}, {1023, 2, false, false}, {513, 3, false, false}, {5, 4, false, false}};
    int chunks = 0, pchunks = 0;
    for (auto& t : ts) {
        t.first = chunks;
        t.chunks = (t.n + ach::OPT_CHUNK - 1) / ach::OPT_CHUNK;
        chunks += t.chunks;
        if (t.flag != 4) pchunks = chunks;
    }
    const size_t all = size_t(chunks) * ach::OPT_CHUNK, par = size_t(pchunks) * ach::OPT_CHUNK;
    auto arena = [](size_t n) { return std::unique_ptr<float, void (*)(void*)>(static_cast<float*>(std::aligned_alloc(16, n * sizeof(float))), std::free); };
    auto state = arena(all), ema = arena(all), grad = arena(par), m1 = arena(par), m2 = arena(par);
    std::vector<int> flags(chunks), t(pchunks, 0);
    std::vector<float> before(all);
    std::unique_ptr<double[]> hyper(new double[ach::OPT_HYPER]);
    for (size_t i = 0; i < all; ++i) state.get()[i] = ema.get()[i] = 0.f;
    for (size_t i = 0; i < par; ++i) grad.get()[i] = m1.get()[i] = m2.get()[i] = 0.f;
    unsigned seed = 12345u;
    auto rnd = [&] { seed = seed * 1664525u + 1013904223u; return float(int(seed >> 8) % 2001 - 1000) * 1e-3f; };
    for (auto& x : ts)
        for (int i = 0; i < x.n; ++i) state.get()[size_t(x.first) * ach::OPT_CHUNK + i] = ema.get()[size_t(x.first) * ach::OPT_CHUNK + i] = rnd();
    for (size_t i = 0; i < all; ++i) before[i] = state.get()[i];
    for (int g = 0; g < 3; ++g) { hyper[ach::OPT_LR + g] = 1e-2; hyper[ach::OPT_WD + g] = g == 1 ? 5e-2 : 0.0; }
    hyper[ach::OPT_EMA_DECAY] = 0.9999; hyper[ach::OPT_EMA_TAU] = 2000.0; hyper[ach::OPT_UPDATES] = 3000.0; hyper[ach::OPT_D] = 0.0;

    for (int s = 0; s < 4; ++s) {
        for (auto& x : ts) {
            const bool active = x.flag <= 2 && !x.never && (!x.late || s >= 2);
            for (int c = 0; c < x.chunks; ++c) flags[x.first + c] = x.flag | (active ? ach::OPT_ACTIVE : 0);
            if (x.flag <= 2)
                for (int i = 0; i < x.n; ++i) grad.get()[size_t(x.first) * ach::OPT_CHUNK + i] = active ? rnd() : 0.f;
        }
        double* const hy = hyper.get();                 // (a launch captures its arguments by copy)
        if (with_ema) ACH_LAUNCH(ach::optim_tick_kernel, dim3(1), dim3(64), nullptr, hy);
        ach::OptimStepParams p{state.get(), with_ema ? ema.get() : nullptr, grad.get(), mu != 0.f || kind != ach::OPT_SGD ? m1.get() : nullptr,
                               kind != ach::OPT_SGD ? m2.get() : nullptr, flags.data(), kind != ach::OPT_SGD ? t.data() : nullptr, hyper.get(), chunks, pchunks, kind, nesterov,
                               mu, 0.937, 0.999, 1e-8};
        // two grids: one workgroup per four chunks, and a single workgroup that walks all chunks in its grid-stride loop (alternating)
        ACH_LAUNCH(ach::optim_step_kernel, dim3(unsigned(s % 2 ? 1 : (chunks + 3) / 4)), dim3(256), nullptr, p);
    }
    if (with_ema && hyper[ach::OPT_UPDATES] != 3004.0) return fail("updates", kind, 0);
    for (auto& x : ts) {
        const size_t a = size_t(x.first) * ach::OPT_CHUNK;
        for (size_t i = x.n; i < size_t(x.chunks) * ach::OPT_CHUNK; ++i) {
            if (state.get()[a + i] != 0.f || ema.get()[a + i] != 0.f) return fail("padding of state / ema", kind, long(a + i));
            if (x.flag != 4 && (grad.get()[a + i] != 0.f || m1.get()[a + i] != 0.f || m2.get()[a + i] != 0.f)) return fail("padding of grad / m1 / m2", kind, long(a + i));
        }
        const bool frozen = x.never || x.flag >= 3;
        int moved = 0;
        for (int i = 0; i < x.n; ++i) {
            if (!(state.get()[a + i] == state.get()[a + i]) || !(ema.get()[a + i] == ema.get()[a + i])) return fail("not a number", kind, long(a + i));
            moved += state.get()[a + i] != before[a + i];
        }
        if (frozen && moved) return fail("a parameter without a gradient, in no group, or a buffer moved", kind, long(a));
        if (!frozen && !moved) return fail("an active parameter did not move", kind, long(a));
        if (kind != ach::OPT_SGD && x.flag <= 2)
            for (int c = 0; c < x.chunks; ++c)
                if (t[x.first + c] != (x.never ? 0 : x.late ? 2 : 4)) return fail("step count", kind, x.first + c);
    }
    return 0;
}
}  // namespace

int main() {
    int rc = run(ach::OPT_SGD, 0.937f, 1, true);
    rc |= run(ach::OPT_SGD, 0.937f, 0, true);
    rc |= run(ach::OPT_SGD, 0.f, 0, false);
    rc |= run(ach::OPT_ADAM, 0.f, 0, true);
    rc |= run(ach::OPT_ADAMW, 0.f, 0, true);
    if (rc == 0) std::printf("optim_main: ok\n");
    return rc;
}
