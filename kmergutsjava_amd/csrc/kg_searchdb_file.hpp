// kg_searchdb_file.hpp -- the file form of a kg_searchdb (include/kmerguts_hip.h states it field by field): the header's layout,
// the checksum, and searchdb_file_check, which finds the first thing that is wrong with a file image.  Host code without a HIP
// call, so that a stand-alone program can run it under a sanitizer; kg_host_searchdb.hpp is its user in the library.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

namespace kgfile {

constexpr uint64_t kHeaderBytes = 448, kAlign = 64, kChecked = 360;
constexpr uint32_t kVersion = 1;
constexpr int kSections = 6;
enum : int { kSecOffsets = 0, kSecResidues = 1, kSecPairs = 2, kSecValues = 3, kSecStarts = 4, kSecNames = 5 };
constexpr char kMagic[9] = "KGSRCHDB";
constexpr int64_t kMaxLen = 1ll << 24, kMaxProteins = 1ll << 29;
// header fields
enum : size_t { kAtVersion = 8, kAtHeaderBytes = 12, kAtTargets = 16, kAtResidues = 24, kAtPairs = 32, kAtKmers = 40, kAtWindows = 48,
                kAtNamesBytes = 56, kAtHasSeeds = 64, kAtHasMask = 68, kAtSeeds = 72, kAtMask = 120, kAtMaskStats = 136, kAtSections = 216,
                kAtChecksum = 360 };

inline uint64_t rd64(const uint8_t *p) { uint64_t v = 0; for (int b = 7; b >= 0; b--) v = v << 8 | p[b]; return v; }
inline uint32_t rd32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void wr64(uint8_t *p, uint64_t v) { for (int b = 0; b < 8; b++) p[b] = (uint8_t)(v >> (8 * b)); }
inline void wr32(uint8_t *p, uint32_t v) { for (int b = 0; b < 4; b++) p[b] = (uint8_t)(v >> (8 * b)); }
inline uint64_t round_up(uint64_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

// (sum of w_i * (2 i + 1) + n) mod 2^64 over the little-endian 64-bit words of p[0 .. n) padded with zero bytes.  Four partial
// sums: the loop is bound by memory, not by the multiplier's latency.
inline uint64_t checksum(const uint8_t *p, uint64_t n)
{
    uint64_t s[4] = {0, 0, 0, 0};
    const uint64_t words = n / 8;
    uint64_t i = 0;
    for (; i + 4 <= words; i += 4)
        for (int k = 0; k < 4; k++) {
            uint64_t w;
            memcpy(&w, p + (i + k) * 8, 8);             // (little-endian hosts: the library's only ones)
            s[k] += w * (2 * (i + k) + 1);
        }
    for (; i < words; i++) s[0] += rd64(p + i * 8) * (2 * i + 1);
    if (n % 8) {
        uint8_t last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(last, p + words * 8, n % 8);
        s[0] += rd64(last) * (2 * words + 1);
    }
    return s[0] + s[1] + s[2] + s[3] + n;
}

struct Layout {
    int64_t n_db = 0, residues = 0, pairs = 0, kmers = 0, windows = 0, names_bytes = 0;
    uint32_t has_seeds = 0, has_mask = 0;
    uint64_t at[kSections] = {}, bytes[kSections] = {}, sum[kSections] = {};
    uint64_t file_bytes = 0;
};

// the sections' bytes and places that the counts imply
inline void lay_out(Layout &l)
{
    l.bytes[kSecOffsets] = ((uint64_t)l.n_db + 1) * 8;
    l.bytes[kSecResidues] = (uint64_t)l.residues;
    l.bytes[kSecPairs] = (uint64_t)l.pairs * 8;
    l.bytes[kSecValues] = (uint64_t)l.pairs * 4;
    l.bytes[kSecStarts] = ((uint64_t)l.kmers + 1) * 4;
    l.bytes[kSecNames] = (uint64_t)l.names_bytes;
    uint64_t at = kHeaderBytes;
    for (int k = 0; k < kSections; k++) {
        l.at[k] = at;
        at = round_up(at + l.bytes[k]);
    }
    l.file_bytes = at;
}

inline std::string num(uint64_t v) { return std::to_string(v); }

// The first thing that is wrong with the image file[0 .. n), or "" and the layout.  verify: the section checksums are computed.
inline std::string searchdb_file_check(const uint8_t *file, uint64_t n, bool verify, Layout *out)
{
    static const char *const sec_name[kSections] = {"offsets", "residues", "pairs", "values", "run starts", "names"};
    if (n < kHeaderBytes) return "the file has " + num(n) + " bytes, fewer than the header's " + num(kHeaderBytes);
    if (memcmp(file, kMagic, 8) != 0) return "wrong magic: not a kg_searchdb file";
    if (rd32(file + kAtVersion) != kVersion) return "wrong version: " + num(rd32(file + kAtVersion)) + ", this library reads version " + num(kVersion);
    if (rd32(file + kAtHeaderBytes) != kHeaderBytes) return "wrong header bytes: " + num(rd32(file + kAtHeaderBytes)) + ", not " + num(kHeaderBytes);
    if (rd64(file + kAtChecksum) != checksum(file, kChecked)) return "header checksum mismatch";
    for (uint64_t k = kAtChecksum + 8; k < kHeaderBytes; k++)
        if (file[k]) return "header byte " + num(k) + " is not 0";
    Layout l;
    l.n_db = (int64_t)rd64(file + kAtTargets);
    l.residues = (int64_t)rd64(file + kAtResidues);
    l.pairs = (int64_t)rd64(file + kAtPairs);
    l.kmers = (int64_t)rd64(file + kAtKmers);
    l.windows = (int64_t)rd64(file + kAtWindows);
    l.names_bytes = (int64_t)rd64(file + kAtNamesBytes);
    l.has_seeds = rd32(file + kAtHasSeeds);
    l.has_mask = rd32(file + kAtHasMask);
    if (l.n_db < 0 || l.n_db >= kMaxProteins) return "targets out of range: " + std::to_string(l.n_db);
    if (l.residues < 0 || l.residues > l.n_db * (kMaxLen - 1)) return "residues out of range: " + std::to_string(l.residues);
    if (l.windows < 0 || l.windows > l.residues * 4) return "valid windows out of range: " + std::to_string(l.windows);
    if (l.pairs < 0 || l.pairs > l.windows || l.pairs >= (1ll << 32)) return "pairs out of range: " + std::to_string(l.pairs);
    if (l.kmers < 0 || l.kmers > l.pairs || (l.kmers == 0) != (l.pairs == 0)) return "k-mers out of range: " + std::to_string(l.kmers);
    if (l.names_bytes < 0 || (uint64_t)l.names_bytes > n) return "names bytes out of range: " + std::to_string(l.names_bytes);
    if (l.has_seeds > 1 || l.has_mask > 1) return "the seeds / mask flags must be 0 or 1";
    lay_out(l);
    for (int k = 0; k < kSections; k++) {
        const uint8_t *e = file + kAtSections + 24 * k;
        l.sum[k] = rd64(e + 16);
        if (rd64(e + 8) != l.bytes[k])
            return std::string("section ") + sec_name[k] + ": " + num(rd64(e + 8)) + " bytes, the counts give " + num(l.bytes[k]);
        if (rd64(e) != l.at[k]) return std::string("section ") + sec_name[k] + ": at " + num(rd64(e)) + ", the layout gives " + num(l.at[k]);
    }
    if (n != l.file_bytes) return "the file has " + num(n) + " bytes, the header gives " + num(l.file_bytes);
    for (int k = 0; k < kSections; k++) {
        if (verify && checksum(file + l.at[k], l.bytes[k]) != l.sum[k]) return std::string("section ") + sec_name[k] + ": checksum mismatch";
        const uint64_t end = l.at[k] + l.bytes[k], next = k + 1 < kSections ? l.at[k + 1] : l.file_bytes;
        for (uint64_t b = end; b < next; b++)
            if (file[b]) return std::string("padding behind section ") + sec_name[k] + " is not 0";
    }
    const uint8_t *off = file + l.at[kSecOffsets];
    if (rd64(off) != 0) return "offsets[0] is not 0";
    for (int64_t p = 0; p < l.n_db; p++) {
        const int64_t len = (int64_t)rd64(off + 8 * (p + 1)) - (int64_t)rd64(off + 8 * p);
        if (len < 0) return "protein " + std::to_string(p) + ": offsets decrease";
        if (len >= kMaxLen) return "protein " + std::to_string(p) + ": 2^24 or more characters";
    }
    if ((int64_t)rd64(off + 8 * l.n_db) != l.residues) return "the last offset is not the residue count";
    if (rd32(file + l.at[kSecStarts] + 4 * (uint64_t)l.kmers) != (uint64_t)l.pairs) return "the last run start is not the pair count";
    *out = l;
    return "";
}

}  // namespace kgfile
