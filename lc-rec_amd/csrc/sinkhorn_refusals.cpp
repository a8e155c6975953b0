// Stand-alone check of the host code in front of the grouped Sinkhorn launches, for a build with that code under AddressSanitizer
// + UBSan (`make sinkhorn_refusals && ./sinkhorn_refusals`): every refusal of lcrec_sinkhorn_assign comes back with its code and
// a text that names the entry point before anything touches a device, and lcrec_debug_sinkhorn_groups_plan (the function the
// call launches by) walks group tables on exact-size heap buffers, the rule for a group whose LDS request would exceed a
// workgroup's 160 KB included.  It runs on a build host without a device.  Not part of liblcrec_hip.so, never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

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

struct Assign {
    const float *r, *cb; int64_t n = 12; int e = 32, K = 16; const int64_t *offs; int G = 3; double eps = 0.003; int iters = 50;
    int64_t *idx; void *ws; size_t wsb = 0;
    int call() const { return lcrec_sinkhorn_assign(r, n, e, cb, K, offs, G, eps, iters, idx, 1, ws, wsb, nullptr, nullptr, nullptr); }
};

int main()
{
    std::vector<double> store(64);
    float *f32 = reinterpret_cast<float *>(store.data());
    int64_t *i64 = reinterpret_cast<int64_t *>(store.data() + 32);
    // the tables live in exact-size heap buffers: a walk past offs[G] is a sanitizer report
    std::vector<int64_t> good = {0, 2, 7, 12}, down = {0, 7, 2, 12}, low = {-1, 2, 7, 12}, high = {0, 2, 7, 13};

    // ---- lcrec_sinkhorn_assign
    const char *who = "sinkhorn_assign";
    Assign ok;
    ok.r = ok.cb = f32; ok.idx = i64; ok.offs = good.data(); ok.ws = store.data();
    ok.wsb = lcrec_sinkhorn_assign_workspace(ok.n, ok.K, good.data(), ok.G);
    Assign a;
    a = ok; a.r = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.cb = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.offs = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.idx = nullptr; expect(a.call(), LCREC_EINVAL, who, "NULL pointer");
    a = ok; a.e = 48; expect(a.call(), LCREC_EUNSUPPORTED, who, "e_dim=48");
    a = ok; a.e = 0; expect(a.call(), LCREC_EUNSUPPORTED, who, "e_dim=0");
    a = ok; a.K = 0; expect(a.call(), LCREC_EINVAL, who, "bad G/K/iters/eps");
    a = ok; a.iters = 0; expect(a.call(), LCREC_EINVAL, who, "bad G/K/iters/eps");
    a = ok; a.eps = 0.0; expect(a.call(), LCREC_EINVAL, who, "bad G/K/iters/eps");
    a = ok; a.eps = -0.003; expect(a.call(), LCREC_EINVAL, who, "bad G/K/iters/eps");
    a = ok; a.eps = __builtin_nan(""); expect(a.call(), LCREC_EINVAL, who, "bad G/K/iters/eps");
    a = ok; a.G = -1; expect(a.call(), LCREC_EINVAL, who, "bad G/K/iters/eps");
    a = ok; a.offs = low.data(); expect(a.call(), LCREC_EINVAL, who, "outside [0, n]");
    a = ok; a.offs = high.data(); expect(a.call(), LCREC_EINVAL, who, "outside [0, n]");
    a = ok; a.offs = down.data(); expect(a.call(), LCREC_EINVAL, who, "not ascending");
    a = ok; a.wsb = ok.wsb - 1; expect(a.call(), LCREC_EWORKSPACE, who, "workspace");
    a = ok; a.ws = nullptr; expect(a.call(), LCREC_EWORKSPACE, who, "workspace");
    a = ok; a.n = 0; a.r = nullptr; expect_true(a.call() == LCREC_OK, "sinkhorn_assign: no rows is not an error");
    a = ok; a.G = 0; a.offs = nullptr; expect_true(a.call() == LCREC_OK, "sinkhorn_assign: no groups is not an error");
    {
        // the debug entry shares the checks, and wants its two outputs together
        const int rc = lcrec_debug_sinkhorn_groups(f32, 12, 32, f32, 16, good.data(), 3, 0.003, 50, i64, 1, store.data(), ok.wsb, nullptr, nullptr,
                                                   nullptr, i64, nullptr);
        expect(rc, LCREC_EINVAL, who, "given together");
        expect(lcrec_debug_sinkhorn_groups(f32, 12, 32, f32, 16, down.data(), 3, 0.003, 50, i64, 1, store.data(), ok.wsb, nullptr, nullptr, nullptr,
                                           nullptr, nullptr), LCREC_EINVAL, who, "not ascending");
    }

    // ---- lcrec_debug_sinkhorn_groups_plan
    who = "debug_sinkhorn_groups_plan";
    lcrec_sinkhorn_groups_plan plan;
    expect(lcrec_debug_sinkhorn_groups_plan(16, nullptr, 3, 1, &plan, nullptr), LCREC_EINVAL, who, "NULL pointer");
    expect(lcrec_debug_sinkhorn_groups_plan(16, good.data(), 3, 1, nullptr, nullptr), LCREC_EINVAL, who, "NULL pointer");
    expect(lcrec_debug_sinkhorn_groups_plan(0, good.data(), 3, 1, &plan, nullptr), LCREC_EINVAL, who, "bad G/K");
    expect(lcrec_debug_sinkhorn_groups_plan(16, good.data(), -1, 1, &plan, nullptr), LCREC_EINVAL, who, "bad G/K");
    expect(lcrec_debug_sinkhorn_groups_plan(16, down.data(), 3, 1, &plan, nullptr), LCREC_EINVAL, who, "not ascending");
    expect(lcrec_debug_sinkhorn_groups_plan(16, low.data(), 3, 1, &plan, nullptr), LCREC_EINVAL, who, "outside [0, n]");
    {
        // every class, an empty group, the slab and a batch-sized group at K = 16, routes in an exact-size buffer
        const int64_t sizes[] = {3, 0, 200, 300, 4097, 1000, 1025, 1030, 128};
        const int G = (int)(sizeof sizes / sizeof sizes[0]);
        std::vector<int64_t> offs(G + 1);
        offs[0] = 5;
        for (int g = 0; g < G; ++g) offs[g + 1] = offs[g] + sizes[g];
        std::vector<lcrec_sinkhorn_group_route> route(G);
        for (int ctx = 0; ctx < 2; ++ctx) {
            expect_true(lcrec_debug_sinkhorn_groups_plan(16, offs.data(), G, ctx, &plan, route.data()) == LCREC_OK, "plan: a mixed table");
            const int want_cls[] = {0, -1, 1, 2, 5, 3, 4, 4, 0}, want_pos[] = {0, -1, 2, 3, -1, 4, 5, 6, 1};
            for (int g = 0; g < G; ++g)
                expect_true(route[g].cls == want_cls[g] && route[g].position == want_pos[g], "plan: a group's class and position");
            expect_true(route[6].slab_offset == 0 && route[7].slab_offset == 1025 * 16 + 1026 + 16, "plan: cumulative slab offsets");
            expect_true(plan.slab_ok == 1 && plan.slab_doubles == (1025 * 16 + 1026 + 16) + (1030 * 16 + 1030 + 16), "plan: slab doubles");
            expect_true(plan.batch_groups == 1 && plan.batch_biggest == 4097 && plan.table_groups == 7, "plan: batch and table counts");
            expect_true(plan.transport == (ctx ? LCREC_SK_TABLE_RING : LCREC_SK_TABLE_SYNCHRONOUS) && plan.fork_mask == (ctx ? 3 : 0),
                        "plan: transport and fork mask");
            expect_true(plan.cls[0].groups == 2 && plan.cls[0].maxg == 128 && plan.cls[0].lds_bytes == (128 * 16 + 128 + 16) * 8 &&
                        !plan.cls[0].set_attribute && plan.cls[0].threads == 256 && !strcmp(plan.cls[0].label, "sinkhorn_tiny"), "plan: class 0");
            expect_true(plan.cls[3].groups == 1 && plan.cls[3].set_attribute && !strcmp(plan.cls[3].label, "sinkhorn_small"), "plan: class 3");
            expect_true(plan.cls[4].groups == 2 && plan.cls[4].lds_bytes == 0 && plan.cls[4].threads == 1024 && plan.cls[4].table_first == 5 &&
                        !strcmp(plan.cls[4].label, "sinkhorn_slab"), "plan: class 4");
            expect_true((size_t)plan.workspace_bytes == lcrec_sinkhorn_assign_workspace(offs[G], 16, offs.data(), G), "plan: workspace");
        }
        expect_true(lcrec_debug_sinkhorn_groups_plan(16, offs.data(), G, 1, &plan, nullptr) == LCREC_OK && plan.table_groups == 7, "plan: no routes");
    }
    {
        // the oversized-LDS rule: four rows at K = 4096 meet the class-3 bound, but (4 * 4096 + 4 + 4096) * 8 + 64 B > 160 KB
        std::vector<int64_t> offs = {0};
        for (int g = 0; g < 8; ++g) offs.push_back(offs.back() + 4);
        std::vector<lcrec_sinkhorn_group_route> route(8);
        expect_true(lcrec_debug_sinkhorn_groups_plan(4096, offs.data(), 8, 1, &plan, route.data()) == LCREC_OK, "plan: K = 4096");
        expect_true(plan.cls[3].groups == 0 && plan.cls[4].groups == 8 && plan.slab_ok == 1 && route[7].cls == LCREC_SK_CLASS_SLAB, "plan: K = 4096, g = 4 is a slab group");
        expect_true(lcrec_debug_sinkhorn_groups_plan(4093, offs.data(), 8, 1, &plan, route.data()) == LCREC_OK && plan.cls[3].groups == 8 &&
                    plan.cls[3].lds_bytes + 64 <= 160 * 1024 && plan.cls[3].lds_bytes + 64 > 160 * 1024 - 64, "plan: K = 4093, g = 4 still fits LDS");
        int64_t lone[2] = {0, 4};
        expect_true(lcrec_debug_sinkhorn_groups_plan(4096, lone, 1, 0, &plan, route.data()) == LCREC_OK && plan.batch_groups == 1 &&
                    plan.table_groups == 0 && plan.transport == LCREC_SK_TABLE_NONE && route[0].cls == LCREC_SK_CLASS_BATCH, "plan: alone it takes the batch path");
        // ... where K > 1024 is refused with a message before any launch (no device on this host: nothing else could come back)
        Assign big = ok;
        big.K = 4096; big.n = 4; big.G = 1; big.offs = lone;
        big.wsb = lcrec_sinkhorn_assign_workspace(4, 4096, lone, 1);
        std::vector<char> room(big.wsb);
        big.ws = room.data();
        expect(big.call(), LCREC_EUNSUPPORTED, "sinkhorn", "K=4096 > 1024");
    }
    printf("%d checks, %d failed\n", checks, failures);
    return failures ? 1 : 0;
}
