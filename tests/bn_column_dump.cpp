// The staging decision of the BN254 Fr host-pointer entries (csrc/bn_column.h, bncol::stage_plan) in a program of its own, so that
// tests/test_bn128_hints_cpu.py can run it under the address and undefined-behaviour sanitizers: walks chosen sets of columns, checks
//   1  every non-empty column lies inside exactly one staged range (and an empty one in none)
//   2  no two staged ranges meet -- but two ranges that are both only read may: bn_column.h keeps such columns two copies
//   3  a range holding a written column is copied back whole
//   4  a range with only read columns is never copied back
//   5  a taken range (not uploaded) holds exactly one column, and that column is written, not read and has stride 1
// and prints one line per case,
//     stage <case> words=<staging buffer> | range +<first byte - A> words=<w> up=<0|1> down=<0|1> ... | col <range or -> +<word in it> ...
// Exits non-zero on a broken invariant.
#include <stdio.h>
#include "bn_column.h"

using bncol::Col;

static const uintptr_t A = 1 << 20;                  // the section's first byte; E: one element
static const uint64_t E = 32;

static int check(const char *name, const Col *c, uint32_t n) {
    const bncol::StagePlan p = bncol::stage_plan(c, n);
    int rc = 0;
    auto bad = [&](const char *what) { fprintf(stderr, "%s: %s\n", name, what); rc = 1; };
    auto end = [&](uint32_t k) { return c[k].ptr + 8 * bncol::span_words(c[k].n, c[k].stride); };
    auto rend = [&](uint32_t r) { return p.range[r].lo + 8 * p.range[r].words; };
    uint64_t words = 0;
    for (uint32_t r = 0; r < p.nRanges; r++) {
        uint32_t members = 0, written = 0, taken_ok = 0;
        for (uint32_t k = 0; k < n; k++) {
            if (p.of[k] != r) continue;
            members++;
            written += c[k].written;
            taken_ok += c[k].written && !c[k].read && c[k].stride == 1;
        }
        if (!members || !p.range[r].words) bad("an empty range");
        if (p.range[r].download != (written > 0)) bad(written ? "a written column is not copied back" : "a range of read columns is copied back");
        if (!p.range[r].upload && !(members == 1 && taken_ok == 1)) bad("a taken range holds more than one written, unread column of stride 1");
        for (uint32_t q = r + 1; q < p.nRanges; q++)
            if ((p.range[r].download || p.range[q].download) && !(rend(r) <= p.range[q].lo || rend(q) <= p.range[r].lo)) bad("two staged ranges meet");
        words += p.range[r].words;
    }
    if (words != p.words) bad("the staging buffer is not the sum of the ranges");
    for (uint32_t k = 0; k < n; k++) {
        if (!c[k].n) { if (p.of[k] != bncol::NO_RANGE) bad("an empty column has a range"); continue; }
        const uint32_t r = p.of[k];
        if (r >= p.nRanges) { bad("a column without a range"); continue; }
        if (c[k].ptr < p.range[r].lo || end(k) > rend(r)) bad("a column sticks out of its range");
        if (p.range[r].lo + 8 * p.off[k] != c[k].ptr) bad("a column's offset");
    }
    printf("stage %s words=%llu |", name, (unsigned long long)p.words);
    for (uint32_t r = 0; r < p.nRanges; r++)
        printf(" range +%llu words=%llu up=%d down=%d", (unsigned long long)(p.range[r].lo - A), (unsigned long long)p.range[r].words,
               p.range[r].upload, p.range[r].download);
    printf(" |");
    for (uint32_t k = 0; k < n; k++) {
        if (p.of[k] == bncol::NO_RANGE) printf(" col - +0");
        else printf(" col %u +%llu", p.of[k], (unsigned long long)p.off[k]);
    }
    printf("\n");
    return rc;
}

int main() {
    int rc = 0;
    const bool R = true, W = true, no = false;       // Col: ptr, n, stride, read, written
    const uintptr_t far = A + (1 << 16);
    { const Col c[] = { { A, 100, 1, R, no }, { far, 100, 1, no, W } };  rc |= check("apart", c, 2); }
    { const Col c[] = { { A, 100, 3, R, no }, { far, 100, 3, no, W } };  rc |= check("apart-strided-output", c, 2); }
    { const Col c[] = { { A, 100, 1, R, no }, { A, 100, 1, no, W } };    rc |= check("same-stride-1", c, 2); }
    { const Col c[] = { { A, 100, 3, R, no }, { A, 100, 3, no, W } };    rc |= check("same-stride-3", c, 2); }
    { const Col c[] = { { far, 100, 1, R, no }, { A, 100, 3, no, W }, { A + E, 100, 3, no, W } };      rc |= check("outputs-at-0-and-1", c, 3); }
    { const Col c[] = { { far, 100, 1, R, no }, { A + 2 * E, 100, 3, no, W }, { A, 100, 3, no, W } };  rc |= check("outputs-at-2-and-0", c, 3); }
    { const Col c[] = { { A, 100, 3, R, no }, { A + E, 100, 3, no, W } };  rc |= check("output-among-inputs", c, 2); }
    { const Col c[] = { { A + E, 65, 3, R, no }, { A + 2 * E, 65, 3, R, no }, { A, 65, 3, no, W } };   rc |= check("three-of-one-section", c, 3); }
    { const Col c[] = { { A, 100, 3, R, no }, { A + E * (99 * 3 + 1), 100, 1, no, W } };               rc |= check("touching", c, 2); }
    { const Col c[] = { { A, 0, 1, R, no }, { A, 100, 1, no, W } };      rc |= check("empty-beside", c, 2); }
    { const Col c[] = { { A, 1, 3, R, no }, { A + E, 1, 3, no, W } };    rc |= check("one-row", c, 2); }
    { const Col c[] = { { A, 1, 3, R, no }, { A, 1, 3, no, W } };        rc |= check("one-row-in-place", c, 2); }
    { const Col c[] = { { A, 100, 3, R, W }, { A + E, 60, 3, R, no } };  rc |= check("counts-acc-first", c, 2); }
    { const Col c[] = { { A + E, 100, 3, R, W }, { A, 60, 3, R, no } };  rc |= check("counts-src-first", c, 2); }
    { const Col c[] = { { A, 100, 3, R, no }, { A + E, 100, 3, R, no }, { far, 100, 1, no, W } };      rc |= check("inputs-of-one-section", c, 3); }
    return rc;
}
