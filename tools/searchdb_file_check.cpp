// searchdb_file_check.cpp -- the reader of a kg_searchdb file (kmergutsjava_amd/csrc/kg_searchdb_file.hpp) as a stand-alone host
// program, so that it can run under a sanitizer:
//
//     g++ -std=c++17 -g -fsanitize=address,undefined -I kmergutsjava_amd/csrc -o searchdb_file_check tools/searchdb_file_check.cpp
//     ./searchdb_file_check DB.kgsdb
//
// It checks the file as kg_searchdb_open does, then every single changed byte of it (three changes per byte) and every prefix
// length: each must be refused.  Exit status 0: the file was accepted and every damaged copy refused.
#include <cstdio>
#include <vector>

#include "kg_searchdb_file.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s DB.kgsdb\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[1 << 16];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + got);
    fclose(f);
    kgfile::Layout l;
    std::string wrong = kgfile::searchdb_file_check(file.data(), file.size(), true, &l);
    if (!wrong.empty()) { fprintf(stderr, "%s: %s\n", argv[1], wrong.c_str()); return 1; }
    printf("%s: %lld targets, %lld residues, %lld pairs, %lld k-mers, %zu bytes\n", argv[1], (long long)l.n_db, (long long)l.residues,
           (long long)l.pairs, (long long)l.kmers, file.size());
    size_t accepted = 0, tried = 0;
    for (size_t at = 0; at < file.size(); at++)
        for (uint8_t flip : {(uint8_t)0x01, (uint8_t)0x80, (uint8_t)0xFF}) {
            std::vector<uint8_t> copy(file);            // (a copy of the exact size: a read behind it is the sanitizer's to find)
            copy[at] ^= flip;
            tried++;
            if (kgfile::searchdb_file_check(copy.data(), copy.size(), true, &l).empty()) {
                accepted++;
                fprintf(stderr, "byte %zu ^ 0x%02x was accepted\n", at, flip);
            }
        }
    for (size_t n = 0; n < file.size(); n += n < 1024 ? 1 : 997) {
        std::vector<uint8_t> copy(file.begin(), file.begin() + n);
        tried++;
        if (kgfile::searchdb_file_check(copy.data(), copy.size(), true, &l).empty()) {
            accepted++;
            fprintf(stderr, "the first %zu bytes were accepted\n", n);
        }
    }
    printf("%zu damaged copies, %zu accepted\n", tried, accepted);
    return accepted ? 1 : 0;
}
