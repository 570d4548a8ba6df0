// Stand-alone host program: builds the BN254 Poseidon parameter tables (csrc/bn_params.cpp) for every width t = 2..17 and writes, under the
// directory given as its argument, the three blobs of each width (tNN.elems, tNN.tiles, tNN.consts) and offsets.json with the named offsets
// (-1: the width has no such region).  tests/test_bn_params_cpu.py builds it with the address and undefined-behaviour sanitizers and checks
// what it writes; no device is involved.
#include "bn_params.h"
#include <stdio.h>
#include <string>

static bool write_blob(const std::string &path, const void *p, size_t n) {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s OUTDIR\n", argv[0]); return 2; }
    const std::string dir = argv[1];
    FILE *js = fopen((dir + "/offsets.json").c_str(), "w");
    if (!js) { perror("offsets.json"); return 2; }
    fprintf(js, "{");
    for (int t = 2; t <= 17; t++) {
        bnp::BnHostParams H;
        if (bnp::bn_build_params(t, H) != 0) { fprintf(stderr, "t = %d: %s\n", t, H.error.c_str()); return 1; }
        char stem[16];
        snprintf(stem, sizeof stem, "/t%02d.", t);
        if (!write_blob(dir + stem + "elems", H.elems.data(), H.elems.size() * 32) || !write_blob(dir + stem + "tiles", H.tiles.data(), H.tiles.size()) ||
            !write_blob(dir + stem + "consts", H.consts.data(), H.consts.size() * 32)) { perror("write"); return 2; }
        const char *names[] = { "C8", "M", "S", "V", "W", "Cd", "m00", "Mt", "Dt", "Pt", "Mt0", "St", "MK", "DK", "KR", "KU", "MK0", "C0p", "SK" };
        const size_t offs[] = { H.C8, H.M, H.S, H.V, H.W, H.Cd, H.m00, H.Mt, H.Dt, H.Pt, H.Mt0, H.St, H.MK, H.DK, H.KR, H.KU, H.MK0, H.C0p, H.SK };
        fprintf(js, "%s\n \"%d\": {\"rp\": %d", t > 2 ? "," : "", t, H.rp);
        for (int k = 0; k < 19; k++) fprintf(js, ", \"%s\": %ld", names[k], offs[k] == bnp::BN_ABSENT ? -1L : (long)offs[k]);
        fprintf(js, "}");
    }
    fprintf(js, "\n}\n");
    return fclose(js) == 0 ? 0 : 2;
}
