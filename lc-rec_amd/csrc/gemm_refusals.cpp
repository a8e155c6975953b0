// Stand-alone check of the host code in front of the GEMM launches, for a build with that code under AddressSanitizer + UBSan
// (`make gemm_refusals && ./gemm_refusals`): every refusal of lcrec_linear_forward, lcrec_linear_backward,
// lcrec_linear_backward_weights and lcrec_linear_bn_forward comes back with its code and a text that names the entry point before
// anything touches a device, and the four launch plans (lcrec_debug_linear_*_plan) walk their steps on exact-size heap buffers.  It runs on a build host without a
// device.  Not part of liblcrec_hip.so, never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/lcrec.h"

static int failures = 0, checks = 0;

static void expect(int rc, int want_rc, const char *who, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, who);
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    ++checks;
    if (!ok) ++failures;
}

static void expect_true(bool ok, const char *what)
{
    ++checks;
    if (!ok) { ++failures; printf("FAIL %s\n", what); }
}

struct Forward {
    const float *x, *W, *b, *sc, *sh; int64_t n = 64; int in = 64, out = 64; float *y;
    int call() const { return lcrec_linear_forward(x, n, in, W, b, sc, sh, 1, out, y, nullptr); }
};

struct Backward {
    const float *gy, *x, *W; int64_t n = 64; int in = 64, out = 64; float *gx, *gw; void *ws; size_t wsb = 0;
    int call() const { return lcrec_linear_backward(gy, x, W, n, in, out, gx, gw, ws, wsb, nullptr); }
};

struct BnForward {
    const float *x; int64_t n = 64; int in = 64; const float *isc, *ish; int relu = 1; const float *W, *b; int out = 64; float *t;
    int stats = 1; float *mean, *rstd, *scale, *shift; void *ws; size_t wsb = 1 << 20; unsigned *tickets;
    int call() const
    {
        return lcrec_linear_bn_forward(x, n, in, isc, ish, relu, W, b, out, t, stats, nullptr, nullptr, 1e-5f, 0.1f, nullptr, nullptr, mean, rstd,
                                       scale, shift, ws, wsb, tickets, nullptr);
    }
};

int main()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    float *f32 = reinterpret_cast<float *>(p), *off4 = reinterpret_cast<float *>(p + 4);

    // ---- lcrec_linear_forward
    const char *who = "linear_forward";
    Forward fok;
    fok.x = fok.W = fok.b = fok.sc = fok.sh = f32; fok.y = f32;
    Forward f;
    f = fok; f.x = nullptr; expect(f.call(), LCREC_EINVAL, who, "NULL pointer");
    f = fok; f.W = nullptr; expect(f.call(), LCREC_EINVAL, who, "NULL pointer");
    f = fok; f.y = nullptr; expect(f.call(), LCREC_EINVAL, who, "NULL pointer");
    f = fok; f.n = -1; expect(f.call(), LCREC_EINVAL, who, "bad shape");
    f = fok; f.in = 0; expect(f.call(), LCREC_EINVAL, who, "bad shape");
    f = fok; f.out = -4; expect(f.call(), LCREC_EINVAL, who, "bad shape");
    f = fok; f.in = 12; expect(f.call(), LCREC_EUNSUPPORTED, who, "in_dim=12 is not a multiple of 8");
    f = fok; f.sh = nullptr; expect(f.call(), LCREC_EINVAL, who, "bn_scale and bn_shift");
    f = fok; f.sc = nullptr; expect(f.call(), LCREC_EINVAL, who, "bn_scale and bn_shift");
    f = fok; f.x = off4; expect(f.call(), LCREC_EINVAL, who, "16-byte aligned");
    f = fok; f.W = off4; expect(f.call(), LCREC_EINVAL, who, "16-byte aligned");
    f = fok; f.n = 0; f.x = nullptr; expect_true(f.call() == LCREC_OK, "linear_forward: an empty batch is not an error");

    // ---- lcrec_linear_backward
    who = "linear_backward";
    Backward ok;
    ok.gy = ok.x = ok.W = f32; ok.gx = ok.gw = f32; ok.ws = p;
    Backward a;
    a = ok; a.gy = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.W = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.x = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.gy = off4; expect(a.call(), LCREC_EINVAL, who, "16-byte aligned");
    a = ok; a.x = off4; expect(a.call(), LCREC_EINVAL, who, "16-byte aligned");
    a = ok; a.W = off4; expect(a.call(), LCREC_EINVAL, who, "16-byte aligned");
    a = ok; a.n = -1; expect(a.call(), LCREC_EINVAL, who, "bad shape");
    a = ok; a.in = 0; expect(a.call(), LCREC_EINVAL, who, "bad shape");
    a = ok; a.out = -32; expect(a.call(), LCREC_EINVAL, who, "bad shape");
    a = ok; a.in = 62; expect(a.call(), LCREC_EUNSUPPORTED, who, "in_dim=62");
    a = ok; a.out = 62; expect(a.call(), LCREC_EUNSUPPORTED, who, "out_dim=62");
    a = ok; a.out = 36; expect(a.call(), LCREC_EUNSUPPORTED, who, "out_dim=36 is not a multiple of 32");
    a = ok; a.n = 1 << 20; a.in = 4096; expect(a.call(), LCREC_EUNSUPPORTED, who, "exceed the 2 GiB");
    a = ok; a.in = 32768; a.out = 32768; expect(a.call(), LCREC_EUNSUPPORTED, who, "exceed the 2 GiB");
    // S = 2 at n = 256: the workspace check comes before the dW launch (gx NULL: nothing is launched before it)
    a = ok; a.n = 256; a.gx = nullptr; a.ws = nullptr; expect(a.call(), LCREC_EWORKSPACE, who, "workspace 0 B < required 32768 B");
    a = ok; a.n = 256; a.gx = nullptr; a.wsb = 32767; expect(a.call(), LCREC_EWORKSPACE, who, "workspace 32767 B < required 32768 B");
    a = ok; a.n = 0; a.gy = nullptr; expect_true(a.call() == LCREC_OK, "linear_backward: an empty batch is not an error");

    // ---- lcrec_linear_backward_weights
    who = "linear_backward_weights";
    lcrec_dw_problem good = {f32, f32, f32, 64, 64, 64, nullptr, nullptr, 0, 0};
    std::vector<lcrec_dw_problem> pr(17, good);
    auto call = [&](int count, void *ws, size_t wsb) { return lcrec_linear_backward_weights(pr.data(), count, ws, wsb, nullptr); };
    expect(call(17, p, 1 << 20), LCREC_EINVAL, who, "17 problems");
    expect(call(-1, p, 1 << 20), LCREC_EINVAL, who, "-1 problems");
    expect(lcrec_linear_backward_weights(nullptr, 1, p, 1 << 20, nullptr), LCREC_EINVAL, who, "1 problems");
    expect_true(call(0, nullptr, 0) == LCREC_OK, "linear_backward_weights: no problem is not an error");
    pr[1] = good; pr[1].n = 0; expect(call(2, p, 1 << 20), LCREC_EUNSUPPORTED, who, "problem 1: n=0");
    pr[1] = good; pr[1].in_dim = 62; expect(call(2, p, 1 << 20), LCREC_EUNSUPPORTED, who, "problem 1: n=64 in=62");
    pr[1] = good; pr[1].out_dim = -4; expect(call(2, p, 1 << 20), LCREC_EUNSUPPORTED, who, "out=-4");
    pr[1] = good; pr[1].n = 1 << 20; pr[1].in_dim = 4096; expect(call(2, p, 1 << 20), LCREC_EUNSUPPORTED, who, "problem 1 exceeds the 2 GiB");
    pr[1] = good; pr[1].x_scale = f32; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "problem 1: x_scale and x_shift go together");
    pr[1] = good; pr[1].x_shift = f32; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "x_scale and x_shift go together");
    pr[1] = good; pr[1].gy = nullptr; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "NULL pointer in problem 1");
    pr[1] = good; pr[1].x = nullptr; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "NULL pointer in problem 1");
    pr[1] = good; pr[1].gw = nullptr; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "NULL pointer in problem 1");
    pr[1] = good; pr[1].gy = off4; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "operands must be 16-byte aligned");
    pr[1] = good; pr[1].gw = off4; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "operands must be 16-byte aligned");
    pr[1] = good; pr[1].x_scale = off4; pr[1].x_shift = f32; expect(call(2, p, 1 << 20), LCREC_EINVAL, who, "x_scale / x_shift must be 16-byte aligned");
    pr[1] = good; pr[1].splits = 2;        // two runs: [2][64][64] floats of workspace
    expect(call(2, nullptr, 0), LCREC_EWORKSPACE, who, "workspace 0 B < required 32768 B");
    expect(call(2, p, 32767), LCREC_EWORKSPACE, who, "workspace 32767 B < required 32768 B");
    expect(call(2, nullptr, 32768), LCREC_EWORKSPACE, who, "required 32768 B");

    // ---- lcrec_linear_bn_forward
    who = "linear_bn_forward";
    BnForward bok;
    bok.x = bok.isc = bok.ish = bok.W = bok.b = f32; bok.t = bok.mean = bok.rstd = bok.scale = bok.shift = f32; bok.ws = p;
    bok.tickets = reinterpret_cast<unsigned *>(p);
    BnForward b;
    b = bok; b.x = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL pointer");
    b = bok; b.W = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL pointer");
    b = bok; b.t = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL pointer");
    b = bok; b.ish = nullptr; expect(b.call(), LCREC_EINVAL, who, "in_scale and in_shift go together");
    b = bok; b.isc = nullptr; expect(b.call(), LCREC_EINVAL, who, "in_scale and in_shift go together");
    b = bok; b.n = 0; expect(b.call(), LCREC_EINVAL, who, "bad shape");
    b = bok; b.in = 0; expect(b.call(), LCREC_EINVAL, who, "bad shape");
    b = bok; b.out = 0; expect(b.call(), LCREC_EINVAL, who, "bad shape");
    b = bok; b.in = 40; expect(b.call(), LCREC_EUNSUPPORTED, who, "in_dim=40 must be a multiple of 32");
    b = bok; b.out = 62; expect(b.call(), LCREC_EUNSUPPORTED, who, "out_dim=62 of 4");
    b = bok; b.n = 1 << 17; b.out = 1024; expect(b.call(), LCREC_EUNSUPPORTED, who, "sized for training batches");
    b = bok; b.out = 4100; expect(b.call(), LCREC_EUNSUPPORTED, who, "sized for training batches");
    b = bok; b.n = 1 << 19; b.in = 1024; b.out = 4; expect(b.call(), LCREC_EUNSUPPORTED, who, "sized for training batches");
    b = bok; b.n = 1; expect(b.call(), LCREC_EINVAL, who, "more than 1 row (n=1)");
    b = bok; b.x = off4; expect(b.call(), LCREC_EINVAL, who, "16-byte aligned");
    b = bok; b.W = off4; expect(b.call(), LCREC_EINVAL, who, "16-byte aligned");
    b = bok; b.isc = off4; expect(b.call(), LCREC_EINVAL, who, "16-byte aligned");
    b = bok; b.mean = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL statistics output or tickets");
    b = bok; b.rstd = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL statistics output or tickets");
    b = bok; b.scale = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL statistics output or tickets");
    b = bok; b.shift = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL statistics output or tickets");
    b = bok; b.tickets = nullptr; expect(b.call(), LCREC_EINVAL, who, "NULL statistics output or tickets");
    b = bok; b.ws = nullptr; expect(b.call(), LCREC_EWORKSPACE, who, "required 768 B");
    b = bok; b.wsb = 767; expect(b.call(), LCREC_EWORKSPACE, who, "workspace 767 B < required 768 B");

    // ---- the plans, on exact-size heap buffers
    {
        std::vector<lcrec_gemm_launch> fwd(4);
        expect_true(lcrec_debug_linear_forward_plan(8200, 384, 4096, 256, fwd.data(), 4) == 2 && fwd[0].family == LCREC_GEMMK_PP &&
                        fwd[0].form == 3 && fwd[0].row0 == 0 && fwd[0].m == 8192 && fwd[0].workgroups == 256 && fwd[0].list_min == 4 &&
                        fwd[0].list_max == 4 && fwd[1].family == LCREC_GEMMK_32x64 && fwd[1].row0 == 8192 && fwd[1].m == 8,
                    "forward plan: a persistent head of 8192 rows and a tail of 8 on the 32 x 64 tiles");
        expect_true(lcrec_debug_linear_forward_plan(70, 32, 68, 256, fwd.data(), 4) == 1 && fwd[0].family == LCREC_GEMMK_32x64 &&
                        fwd[0].tiles == 3 * 2 && fwd[0].form == 0 && fwd[0].list_max == 0,
                    "forward plan: one launch on the 32 x 64 tiles");
        expect_true(lcrec_debug_linear_forward_plan(3336, 384, 3840, 256, fwd.data(), 4) == 1 && fwd[0].form == 3 &&
                        fwd[0].virtual_tiles > fwd[0].tiles && fwd[0].empty_workgroups == 4 && fwd[0].list_min == 0 && fwd[0].list_max == 2,
                    "forward plan: a persistent launch whose tile numbering has holes");
        expect_true(lcrec_debug_linear_forward_plan(0, 384, 4096, 256, fwd.data(), 4) == 0 &&
                        lcrec_debug_linear_forward_plan(0, 384, 4096, 0, nullptr, 0) == 0, "forward plan: empty batch, whatever the rest");
        // (a refused forward plan is a plain code: it leaves the last-error text alone)
        expect_true(lcrec_debug_linear_forward_plan(64, 64, 64, 256, fwd.data(), 3) == LCREC_EINVAL, "forward plan: capacity 3 is refused");
        expect_true(lcrec_debug_linear_forward_plan(64, 64, 64, 0, fwd.data(), 4) == LCREC_EINVAL, "forward plan: 0 CUs are refused");
        expect_true(lcrec_debug_linear_forward_plan(64, 64, 64, 256, nullptr, 4) == LCREC_EINVAL, "forward plan: NULL output is refused");
        const std::string before = lcrec_last_error();
        expect_true(lcrec_debug_linear_forward_plan(64, 12, 64, 256, fwd.data(), 4) == LCREC_EUNSUPPORTED && before == lcrec_last_error(),
                    "forward plan: in_dim = 12 is refused, the last-error text untouched");
        std::vector<lcrec_gemm_launch> out(3);
        expect_true(lcrec_debug_linear_backward_plan(2048, 68, 64, 1, 1, out.data(), 3) == 3, "backward plan: dX, dW, reducer");
        expect_true(out[1].runs == 16 && out[2].family == LCREC_GEMMK_REDUCER && out[2].total4 == 64 * 68 / 4, "backward plan: S = 16");
        expect(lcrec_debug_linear_backward_plan(64, 64, 64, 1, 1, out.data(), 2), LCREC_EINVAL, "linear_backward_plan", "room for 3");
        expect(lcrec_debug_linear_backward_plan(64, 64, 36, 1, 1, out.data(), 3), LCREC_EUNSUPPORTED, "linear_backward", "multiple of 32");
        expect_true(lcrec_debug_linear_backward_plan(0, 64, 64, 1, 1, out.data(), 3) == 0, "backward plan: empty batch");
        std::vector<lcrec_dw_problem> q(16, good);
        for (int i = 0; i < 16; ++i) { q[i].n = 32 * (i + 1); q[i].splits = i % 4; q[i].gy = q[i].x = nullptr; q[i].gw = nullptr; }
        std::vector<lcrec_gemm_launch> rec(32);
        int grids[2] = {0, 0};
        const int got = lcrec_debug_linear_backward_weights_plan(q.data(), 16, rec.data(), 32, grids);
        expect_true(got >= 16 && got <= 32 && grids[0] > 0 && grids[1] > 0, "weights plan: products and reducers");
        int wgs = 0;
        for (int i = 0; i < 16; ++i) { expect_true(rec[i].wg_start == wgs, "weights plan: wg_start"); wgs += rec[i].workgroups; }
        expect_true(wgs == grids[0], "weights plan: grid total");
        expect(lcrec_debug_linear_backward_weights_plan(q.data(), 16, rec.data(), 31, grids), LCREC_EINVAL, "linear_backward_weights_plan", "room for 32");
        std::vector<lcrec_gemm_launch> one(1);
        expect_true(lcrec_debug_linear_bn_forward_plan(7809, 32, 4, 1, 1, one.data()) == 1 && one[0].chunks == 2 && one[0].chunk_row_tiles == 60,
                    "bn forward plan: two merge chunks of 128 x 32 tiles");
        expect_true(lcrec_debug_linear_bn_forward_plan(64, 32, 32, 0, 0, one.data()) == 0, "bn forward plan: neither fold nor statistics");
        expect(lcrec_debug_linear_bn_forward_plan(64, 40, 32, 1, 1, one.data()), LCREC_EUNSUPPORTED, "linear_bn_forward", "in_dim=40");
    }
    printf("gemm_refusals: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
