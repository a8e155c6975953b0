// Stand-alone check of the host code behind --extend, for a build with that code under AddressSanitizer + UBSan
// (`make extend_host_check && ./extend_host_check`).  Two things:
//   1. every argument refusal of lcrec_extend_nearest_free comes back with its code and a text before anything touches a device;
//   2. lcrec_index_json_parse on texts held in EXACT-SIZE heap buffers (so one byte read past the text is a sanitizer report):
//      round trips through lcrec_index_json_format, every truncation point of a valid text, and each malformed kind.
// It runs on a build host without a device.  Not part of liblcrec_hip.so, never loaded into Python.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/lcrec.h"

static int failures = 0, checks = 0;

static void expect(int rc, int want_rc, const char *word)
{
    const char *text = lcrec_last_error();
    const bool ok = rc == want_rc && strstr(text, word) && strstr(text, "extend_nearest_free");
    printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, text);
    ++checks;
    if (!ok) ++failures;
}

static void refusals()
{
    std::vector<double> store(64);
    char *p = reinterpret_cast<char *>(((uintptr_t)store.data() + 15) & ~(uintptr_t)15);
    int64_t *i64 = reinterpret_cast<int64_t *>(p);
    float *f32 = reinterpret_cast<float *>(p);
    int64_t *i64_off4 = reinterpret_cast<int64_t *>(p + 4);
    float *f32_off4 = reinterpret_cast<float *>(p + 4), *f32_off8 = reinterpret_cast<float *>(p + 8);
    const int K3[3] = {48, 48, 48}, K0[3] = {48, 48, 0}, Kbig[3] = {48, 48, 4096}, K1[1] = {2048};
    const int K16[2] = {4, 1900}, K32[2] = {4, 1080};   // levels lcrec_finish_nearest_free takes: the extra array does not fit
    const int es[] = {0, 8, 24, 128, -16};
    char word[64];
    auto f = lcrec_extend_nearest_free;
    expect(f(i64, 8, -1, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "n_frozen=-1");
    expect(f(i64, 8, 9, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "n_frozen=9 (0 .. n=8)");
    expect(f(i64, 8, 3, 3, K3, nullptr, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "resid_last, with 5 new items");
    for (int e : es) {
        snprintf(word, sizeof word, "e_dim=%d", e);
        expect(f(i64, 8, 2, 3, K3, f32, e, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED, word);
    }
    expect(f(i64, 8, 2, 3, K0, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "K[2]=0");
    expect(f(i64, 8, 2, 3, Kbig, f32, 64, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED, "level 2 (K=4096, e=64) does not fit");
    expect(f(i64, 8, 2, 1, K1, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED, "level 0 (K=2048, e=16) does not fit");
    expect(f(i64, 8, 2, 2, K16, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED,
           "level 1 (K=1900, e=16) does not fit in 160 KB of LDS with the frozen-holder counts (167200 B");
    expect(f(i64, 8, 2, 2, K32, f32, 32, f32, i64, i64, 1, i64, nullptr), LCREC_EUNSUPPORTED,
           "level 1 (K=1080, e=32) does not fit in 160 KB of LDS with the frozen-holder counts");
    // ... which the entry without frozen holders passes: it goes on to its next check (here: a NULL pointer)
    {
        const int rc = lcrec_finish_nearest_free(nullptr, 8, 2, K16, f32, 16, f32, i64, i64, 1, i64, nullptr);
        const bool ok = rc == LCREC_EINVAL && strstr(lcrec_last_error(), "finish_nearest_free: NULL pointer");
        printf("%s rc=%d \"%s\"\n", ok ? "ok  " : "FAIL", rc, lcrec_last_error());
        ++checks;
        if (!ok) ++failures;
    }
    expect(f(i64, 8, 2, 0, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "L=0");
    expect(f(i64, 8, 2, 17, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "L=17");
    expect(f(i64, -1, 0, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "n=-1");
    expect(f(i64, (int64_t)1 << 32, 0, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "n=4294967296");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, i64, i64, -1, i64, nullptr), LCREC_EINVAL, "n_buckets=-1");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, i64, i64, (int64_t)1 << 31, i64, nullptr), LCREC_EINVAL, "n_buckets=2147483648");
    expect(f(i64, 8, 2, 3, K3, f32_off8, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32_off4, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "16-byte aligned");
    expect(f(i64_off4, 8, 2, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, i64_off4, i64, 1, i64, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, i64, i64_off4, 1, i64, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, i64, i64, 1, i64_off4, nullptr), LCREC_EINVAL, "8-byte aligned");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, i64, i64, 1, nullptr, nullptr), LCREC_EINVAL, "counters_out is NULL");
    expect(f(i64, 8, 2, 3, nullptr, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "K is NULL");
    expect(f(nullptr, 8, 2, 3, K3, f32, 16, f32, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "NULL pointer");
    expect(f(i64, 8, 2, 3, K3, f32, 16, f32, nullptr, i64, 1, i64, nullptr), LCREC_EINVAL, "NULL pointer");
    expect(f(i64, 8, 2, 3, K3, f32, 16, nullptr, i64, i64, 1, i64, nullptr), LCREC_EINVAL, "NULL pointer");
}

// ---- the parser -------------------------------------------------------------------------------------------------------------
static void note(bool ok, const char *what, long long a = 0, long long b = 0)
{
    ++checks;
    if (ok) return;
    ++failures;
    printf("FAIL %s (%lld, %lld) last error \"%s\"\n", what, a, b, lcrec_last_error());
}

// the parse of `text` from a heap buffer of exactly text.size() bytes into a heap buffer of exactly cap rows
static int64_t parse_exact(const std::string &text, int L, std::vector<int64_t> *rows, int64_t cap)
{
    char *buf = static_cast<char *>(malloc(text.size() ? text.size() : 1));
    memcpy(buf, text.data(), text.size());
    int64_t *out = static_cast<int64_t *>(malloc(cap * L ? (size_t)(cap * L) * sizeof(int64_t) : 1));
    const int64_t got = lcrec_index_json_parse(buf, (int64_t)text.size(), L, out, cap);
    if (rows) rows->assign(out, out + (got > 0 ? got * L : 0));
    free(out);
    free(buf);
    return got;
}

static std::string format_all(const std::vector<int64_t> &idx, int64_t n, int L)
{
    std::string body((size_t)lcrec_index_json_bound(n, L) + 1, '\0');
    const int64_t len = lcrec_index_json_format(idx.data(), n, L, 0, &body[0], (int64_t)body.size());
    if (len < 0) { ++failures; return "{}"; }
    return "{" + body.substr(0, (size_t)len) + "}";
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

static void round_trips()
{
    const int64_t special[] = {0, 9, 10, 99, 100, INT64_MAX, INT64_MAX - 1, 1000000000000000000ll};
    const int Ls[] = {1, 4, 26};
    for (int L : Ls) {
        const int64_t ns[] = {0, 1, 2, 11, 5000};
        for (int64_t n : ns) {
            std::vector<int64_t> idx((size_t)(n * L));
            for (size_t q = 0; q < idx.size(); ++q) {
                const uint64_t r = rng();
                idx[q] = (r & 3) == 0 ? special[(r >> 2) % 8] : (int64_t)((r >> 2) % ((r & 4) ? 300 : 70000));
            }
            const std::string text = format_all(idx, n, L);
            std::vector<int64_t> back;
            const int64_t got = parse_exact(text, L, &back, n);                      // cap == n exactly
            note(got == n && back == idx, "round trip", L, n);
            if (n > 0) {
                const int64_t short_rc = parse_exact(text, L, nullptr, n - 1);        // one row short: refused, nothing past cap written
                note(short_rc == LCREC_EWORKSPACE && strstr(lcrec_last_error(), "cap_items"), "cap_items one short", L, n);
            }
        }
    }
    printf("round trips: L = 1, 4, 26 x n = 0, 1, 2, 11, 5000 (codes 0, 9, 10, 2^63-1, random) done\n");
}

static void malformed()
{
    const std::vector<int64_t> idx = {0, 9, 10, 123, 4, INT64_MAX, 7, 7, 48};
    const std::string good = format_all(idx, 3, 3);
    std::vector<int64_t> back;
    note(parse_exact(good, 3, &back, 3) == 3 && back == idx, "the small text itself");
    for (size_t cut = 0; cut < good.size(); ++cut) {                                  // every truncation point
        const int64_t rc = parse_exact(good.substr(0, cut), 3, nullptr, 3);
        note(rc == LCREC_EINVAL && strstr(lcrec_last_error(), "byte "), "truncation", (long long)cut, rc);
    }
    printf("truncations: %zu prefixes of a %zu-byte text refused\n", good.size(), good.size());
    auto refused = [&](std::string text, const char *what, const char *word, int L = 3) {
        const int64_t rc = parse_exact(text, L, nullptr, 8);
        const bool ok = rc == LCREC_EINVAL && strstr(lcrec_last_error(), word) && strstr(lcrec_last_error(), "byte ");
        printf("%s %-28s rc=%lld \"%s\"\n", ok ? "ok  " : "FAIL", what, (long long)rc, lcrec_last_error());
        ++checks;
        if (!ok) ++failures;
    };
    std::string t = good;
    t[t.find("<b_")  + 1] = 'c';
    refused(t, "a wrong letter", "prefix letter");
    t = good;
    t.replace(t.find("\"1\""), 3, "\"2\"");
    refused(t, "a key out of order", "keys are");
    refused("{\"1\": [\"<a_0>\"]}", "a first key that is not 0", "keys are", 1);
    refused("{\"00\": [\"<a_0>\"]}", "a key with a leading zero", "keys are", 1);
    refused("{\"0\": [\"<a_12345678901234567890>\"]}", "a 20-digit overflow", "64-bit", 1);
    refused("{\"0\": [\"<a_9223372036854775808>\"]}", "2^63", "64-bit", 1);
    refused("{\"0\": [\"<a_-1>\"]}", "a minus sign", "non-negative", 1);
    refused("{\"0\": [\"<a_01>\"]}", "a leading zero", "non-negative", 1);
    refused("{\"0\": [\"<a_>\"]}", "no digits", "non-negative", 1);
    refused(good + "\n", "trailing bytes after }", "end of the text");
    refused(good + "}", "a second }", "end of the text");
    refused("{} ", "trailing bytes after {}", "end of the text");
    refused(" {}", "leading white space", "'{'");
    refused("", "the empty text", "'{'");
    refused("{\"0\":[\"<a_0>\"]}", "compact separators", "\": [", 1);
    refused("{\"0\": [\"<a_0>\",\"<b_1>\"]}", "a compact token separator", "another token", 2);
    refused("{\"0\": [\"<a_0>\"]}", "too few tokens", "another token", 2);
    refused("{\"0\": [\"<a_0>\", \"<b_1>\"]}", "too many tokens", "']'", 1);
    refused("{\"0\": [\"<a_0>\"],\"1\": [\"<a_0>\"]}", "a compact item separator", "', ' or '}'", 1);
    refused("{\"0\": [\"<a_0>\"], }", "a trailing comma", "opening a key", 1);
    note(parse_exact("{}", 3, nullptr, 0) == 0, "{} gives 0 items");
    note(parse_exact("{}", 3, nullptr, 5) == 0, "{} gives 0 items (room to spare)");
    note(lcrec_index_json_parse(nullptr, 2, 3, nullptr, 0) == LCREC_EINVAL, "NULL text");
    note(lcrec_index_json_parse("{}", 2, 0, nullptr, 0) == LCREC_EINVAL, "L = 0");
    note(lcrec_index_json_parse("{}", 2, 27, nullptr, 0) == LCREC_EINVAL, "L = 27");
    note(lcrec_index_json_parse("{}", -1, 3, nullptr, 0) == LCREC_EINVAL, "len < 0");
}

int main()
{
    refusals();
    const int after_refusals = checks;
    round_trips();
    malformed();
    printf("extend_host_check: %d refusal checks, %d parser checks, %d failures\n", after_refusals, checks - after_refusals, failures);
    return failures ? 1 : 0;
}
