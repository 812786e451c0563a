// The host build of csrc/poseidon_dev.h behind a pipe (tests/test_poseidon_group4_host.py compiles this file with the C++ compiler).
//   driver permute OUT | group4 G | group3tail | foldwide      uint64 words on stdin -> uint64 words on stdout, native byte order
// permute, group4, group3tail: states of 12 words -> states of 12 words.  foldwide: triples (al, ah, cl + 2 ch) -> words.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poseidon_dev.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::vector<uint64_t> in;
    uint64_t buf[1536];
    size_t k;
    while ((k = fread(buf, 8, 1536, stdin)) > 0) in.insert(in.end(), buf, buf + k);
    const bool fold = !strcmp(argv[1], "foldwide");
    const int arg = argc > 2 ? atoi(argv[2]) : 0;
    const size_t per = fold ? 3 : 12, n = in.size() / per;
    if (in.size() % per) return 3;
    std::vector<uint64_t> out;
    for (size_t i = 0; i < n; i++) {
        uint64_t* s = &in[i * per];
        if (fold) {
            out.push_back(poseidon_fold_wide(s[0], s[1], s[2] & 1, (s[2] >> 1) & 1));
            continue;
        }
        if (!strcmp(argv[1], "permute")) {
            poseidon_permute_out(s, arg);
        } else if (!strcmp(argv[1], "group4")) {
            if (arg < 0 || arg > 4) return 4;
            poseidon_partial_group4(s, PC::ZKM_POSEIDON_G4_C1[arg], PC::ZKM_POSEIDON_G4_C2[arg], &PC::ZKM_POSEIDON_G4_C3[arg], PC::ZKM_POSEIDON_G4_C4[arg]);
        } else if (!strcmp(argv[1], "group3tail")) {
            poseidon_partial_group<3>(s, PC::ZKM_POSEIDON_G4_TAIL_C12[0], PC::ZKM_POSEIDON_G4_TAIL_C12[1], PC::ZKM_POSEIDON_G4_TAIL_C3);
        } else {
            return 2;
        }
        out.insert(out.end(), s, s + 12);
    }
    return fwrite(out.data(), 8, out.size(), stdout) == out.size() ? 0 : 5;
}
