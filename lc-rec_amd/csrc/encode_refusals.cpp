// Stand-alone check of the host code in front of the encode pass, for a build with that code under AddressSanitizer + UBSan
// (`make encode_refusals && ./encode_refusals`): every refusal of lcrec_debug_encode_assign_plan, of the two workspace queries and of
// lcrec_encode_assign / lcrec_debug_encode_assign comes back with its code and a text that names the argument before anything touches
// a device, and the plan export walks the shapes of tests/encode_cases.py and the production sizes into exact-size heap buffers,
// where its chunks must tile the rows and its buffers must not overlap.  It runs on a build host without a device.  Not part of
// liblcrec_hip.so, never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/lcrec.h"

static int failures = 0, checks = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "encode_assign");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    ++checks;
    if (!ok) ++failures;
}

static void expect_true(bool ok, const char *what)
{
    ++checks;
    if (!ok) { ++failures; printf("FAIL %s\n", what); }
}

struct Shape { const char *name; std::vector<int> dims, K; };

// one plan into exact-size buffers, held to what include/lcrec.h states
static void walk(const Shape &s, int64_t n, int64_t chunk_rows, int pipelines)
{
    const int nl = (int)s.dims.size() - 1, L = (int)s.K.size();
    lcrec_encode_plan *plan = new lcrec_encode_plan;
    int rc = lcrec_debug_encode_assign_plan(n, s.dims.data(), nl, s.K.data(), L, chunk_rows, pipelines, plan, nullptr, 0);
    expect_true(rc == LCREC_OK, "plan: a shape of the table is refused");
    if (rc != LCREC_OK) { delete plan; return; }
    std::vector<lcrec_encode_chunk> chunks((size_t)plan->n_chunks);
    rc = lcrec_debug_encode_assign_plan(n, s.dims.data(), nl, s.K.data(), L, chunk_rows, pipelines, plan, chunks.data(), plan->n_chunks);
    expect_true(rc == LCREC_OK, "plan: the chunk list is refused at its exact capacity");
    const int64_t want = chunk_rows ? chunk_rows : lcrec_encode_assign_chunk_rows();
    const int64_t chunk = want < (n > 0 ? n : 1) ? want : (n > 0 ? n : 1);
    bool ok = plan->n == n && plan->chunk_rows == chunk && plan->n_chunks == (n + chunk - 1) / chunk;
    const int P = plan->n_chunks < pipelines ? (plan->n_chunks > 1 ? (int)plan->n_chunks : 1) : pipelines;
    ok = ok && plan->pipelines == P;
    int64_t row = 0;
    for (int64_t c = 0; c < plan->n_chunks; ++c) {
        const lcrec_encode_chunk &k = chunks[(size_t)c];
        ok = ok && k.row0 == row && k.rows == (c + 1 < plan->n_chunks ? chunk : n - row) && k.pipeline == c % P && k.first_act == 2 * k.pipeline;
        row += k.rows;
    }
    ok = ok && row == n;
    // the ranges: disjoint, aligned, in order, adding up to the total, which both queries return
    int64_t at = 0;
    for (int i = 0; i < LCREC_ENC_ACT_BUFFERS; ++i) { ok = ok && plan->act_offset[i] == at && at % 256 == 0; at += plan->act_bytes; }
    int widest = 1;
    for (int l = 1; l < nl; ++l) widest = s.dims[l] > widest ? s.dims[l] : widest;
    ok = ok && plan->act_bytes == (chunk * widest * 4 + 255) / 256 * 256;
    ok = ok && plan->latent_offset == at && plan->latent_bytes >= (n > 0 ? n : 1) * s.dims[nl] * 4 && plan->latent_bytes % 256 == 0;
    at += plan->latent_bytes;
    ok = ok && plan->rq_offset == at && plan->rq_bytes == (int64_t)lcrec_rq_assign_workspace(n, s.dims[nl], s.K.data(), L) && plan->rq_bytes % 256 == 0;
    at += plan->rq_bytes;
    ok = ok && plan->total_bytes == at;
    ok = ok && (int64_t)lcrec_debug_encode_assign_workspace(n, s.dims.data(), nl, s.K.data(), L, chunk_rows) == at;
    if (chunk_rows == 0) ok = ok && (int64_t)lcrec_encode_assign_workspace(n, s.dims.data(), nl, s.K.data(), L) == at;
    if (!ok) printf("FAIL plan of %s n=%lld chunk_rows=%lld pipelines=%d\n", s.name, (long long)n, (long long)chunk_rows, pipelines);
    expect_true(ok, "plan: chunks or layout");
    delete plan;
}

int main()
{
    const Shape W = {"W", {384, 2048, 128, 64, 32}, {256, 256, 64}}, N1 = {"N1", {64, 32}, {48, 7}}, N3 = {"N3", {128, 96, 48, 16}, {48, 7}};
    const Shape C3 = {"C3", {768, 2048, 1024, 512, 256, 128, 64, 32}, {256, 256, 256, 256}};
    const Shape C4 = {"C4", {4096, 2048, 1024, 512, 256, 128, 64, 32}, {256, 256, 256, 256}};

    // ---- the plan export's refusals
    std::vector<int> dims = {64, 48, 32}, K = {48, 7}, deep(LCREC_MAX_LAYERS + 2, 32);
    lcrec_encode_plan plan;
    std::vector<lcrec_encode_chunk> four(4);
    auto call = [&](int64_t n, const int *d, int nl, const int *k, int L, int64_t chunk_rows, int pipelines, lcrec_encode_plan *p, int64_t cap) {
        return lcrec_debug_encode_assign_plan(n, d, nl, k, L, chunk_rows, pipelines, p, four.data(), cap);
    };
    expect_true(call(100, dims.data(), 2, K.data(), 2, 33, 2, &plan, 4) == LCREC_OK && plan.n_chunks == 4 && four[3].rows == 1 && four[3].pipeline == 1,
                "plan: 100 rows in chunks of 33");
    expect(call(-1, dims.data(), 2, K.data(), 2, 33, 2, &plan, 4), LCREC_EINVAL, "n < 0");
    expect(call(100, dims.data(), 0, K.data(), 2, 33, 2, &plan, 4), LCREC_EINVAL, "n_layers=0");
    expect(call(100, deep.data(), LCREC_MAX_LAYERS + 1, K.data(), 2, 33, 2, &plan, 4), LCREC_EINVAL, "n_layers=17");
    expect(call(100, nullptr, 2, K.data(), 2, 33, 2, &plan, 4), LCREC_EINVAL, "dims");
    expect(call(100, dims.data(), 2, nullptr, 2, 33, 2, &plan, 4), LCREC_EINVAL, "K");
    expect(call(100, dims.data(), 2, K.data(), 0, 33, 2, &plan, 4), LCREC_EINVAL, "L=0");
    expect(call(100, dims.data(), 2, K.data(), 2, -1, 2, &plan, 4), LCREC_EINVAL, "chunk_rows=-1");
    expect(call(100, dims.data(), 2, K.data(), 2, 33, 0, &plan, 4), LCREC_EINVAL, "pipelines=0");
    expect(call(100, dims.data(), 2, K.data(), 2, 33, 3, &plan, 4), LCREC_EINVAL, "pipelines=3");
    expect(call(100, dims.data(), 2, K.data(), 2, 33, 2, &plan, 3), LCREC_EINVAL, "capacity 3");
    expect(call(100, dims.data(), 2, K.data(), 2, 33, 2, nullptr, 4), LCREC_EINVAL, "plan_out");

    // ---- the workspace queries answer 0 for what the plan refuses
    expect_true(lcrec_encode_assign_workspace(100, nullptr, 2, K.data(), 2) == 0 && lcrec_encode_assign_workspace(100, dims.data(), 0, K.data(), 2) == 0 &&
                    lcrec_encode_assign_workspace(100, deep.data(), LCREC_MAX_LAYERS + 1, K.data(), 2) == 0 &&
                    lcrec_encode_assign_workspace(100, dims.data(), 2, nullptr, 2) == 0 && lcrec_encode_assign_workspace(100, dims.data(), 2, K.data(), 0) == 0 &&
                    lcrec_encode_assign_workspace(-1, dims.data(), 2, K.data(), 2) == 0 &&
                    lcrec_debug_encode_assign_workspace(100, dims.data(), 2, K.data(), 2, -1) == 0,
                "workspace queries: 0 for refused arguments");

    // ---- the launch entries: refused before a device is touched
    std::vector<float> store(64);
    float *f32 = store.data();
    const float *ptrs[2] = {f32, f32};
    int64_t idx[4];
    auto launch = [&](const float *x, int64_t n, const int *d, int nl, const float *const *Wp, const int *k, int L, int64_t *out, void *ws, size_t wsb,
                      int64_t chunk_rows) {
        return lcrec_debug_encode_assign(x, n, d, nl, Wp, ptrs, nullptr, nullptr, f32, k, L, out, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f, ws, wsb,
                                         nullptr, nullptr, chunk_rows);
    };
    expect(launch(f32, 100, dims.data(), 2, ptrs, K.data(), 2, idx, f32, 1 << 20, -1), LCREC_EINVAL, "chunk_rows=-1");
    expect(launch(nullptr, 100, dims.data(), 2, ptrs, K.data(), 2, idx, f32, 1 << 20, 33), LCREC_EINVAL, "NULL pointer");
    expect(launch(f32, 100, dims.data(), 2, nullptr, K.data(), 2, idx, f32, 1 << 20, 33), LCREC_EINVAL, "NULL pointer");
    expect(launch(f32, 100, dims.data(), 2, ptrs, K.data(), 2, nullptr, f32, 1 << 20, 33), LCREC_EINVAL, "NULL pointer");
    expect(launch(f32, 100, nullptr, 2, ptrs, K.data(), 2, idx, f32, 1 << 20, 33), LCREC_EINVAL, "NULL pointer");
    expect(launch(f32, -1, dims.data(), 2, ptrs, K.data(), 2, idx, f32, 1 << 20, 33), LCREC_EINVAL, "n < 0");
    expect(launch(f32, 100, dims.data(), 0, ptrs, K.data(), 2, idx, f32, 1 << 20, 33), LCREC_EINVAL, "n_layers=0");
    expect(launch(f32, 100, dims.data(), 2, ptrs, K.data(), 0, idx, f32, 1 << 20, 33), LCREC_EINVAL, "L=0");
    const size_t need = lcrec_debug_encode_assign_workspace(100, dims.data(), 2, K.data(), 2, 33);
    char text[64];
    snprintf(text, sizeof(text), "required %zu B", need);
    expect(launch(f32, 100, dims.data(), 2, ptrs, K.data(), 2, idx, f32, need - 1, 33), LCREC_EWORKSPACE, text);
    expect(launch(f32, 100, dims.data(), 2, ptrs, K.data(), 2, idx, nullptr, need, 33), LCREC_EWORKSPACE, text);
    expect_true(launch(nullptr, 0, dims.data(), 2, nullptr, K.data(), 2, nullptr, nullptr, 0, 33) == LCREC_OK, "encode_assign: an empty batch is not an error");
    expect(lcrec_encode_assign(f32, 100, dims.data(), 2, ptrs, ptrs, nullptr, nullptr, f32, K.data(), 2, idx, nullptr, nullptr, nullptr, nullptr, nullptr, 0.0f,
                               f32, 16, nullptr, nullptr),
           LCREC_EWORKSPACE, "workspace 16 B < required");

    // ---- the plans of the table's shapes (tests/encode_cases.py) and of the production sizes, both pipeline settings
    struct Row { const Shape *s; int64_t n, chunk_rows; };
    const Row rows[] = {{&W, 9200, 0}, {&W, 4096, 5000}, {&N3, 1500, 0}, {&N1, 1500, 4000}, {&W, 8192, 4096}, {&N3, 1500, 500}, {&N1, 1500, 500},
                        {&W, 8193, 4096}, {&W, 9617, 4571}, {&W, 3017, 1000}, {&W, 1037, 257}, {&W, 130, 33}, {&N3, 1490, 33}, {&N1, 1037, 257},
                        {&N1, 5, 1}, {&N3, 5, 1}, {&N1, 1, 0}, {&N1, 0, 0}, {&C3, 1000000, 0}, {&C4, 1250000, 0}, {&C3, 524288, 0}, {&C3, 524289, 0},
                        {&C3, 1000000, 1}};
    for (const Row &r : rows)
        for (int P = 1; P <= LCREC_ENC_PIPES_MAX; ++P) walk(*r.s, r.n, r.chunk_rows, P);

    printf("encode_refusals: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
