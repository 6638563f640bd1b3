// csa_internal.h -- what the archive layer's two translation units share: csa_archive.cpp (the container format, the host paths,
// the sharded Add) and csa_dev_archive.cpp (the device-resident read and write).  The index model, its packing, the header check,
// the plan of an Add and the launchers of csa_dev_kernels.hip.  Nothing here is exported (exports.map).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "../../include/csc_mi355x.h"
#include "../../include/csa_mi355x.h"

// csa_dev_kernels.hip.  launch_gather_extents, launch_frag_pieces / _compare / _slices and launch_frag_fold / _fold_diff launch even
// for an empty table (one workgroup that returns at once).
void launch_gather_extents(const void *pieces, uint32_t npieces, hipStream_t st);
void launch_frag_pieces(const void *pieces, void *sums, uint32_t npieces, bool store, hipStream_t st);
void launch_frag_compare(const void *pieces, void *sums, void *firsts, uint32_t npieces, hipStream_t st);
void launch_frag_slices(const void *pieces, void *sums, uint32_t npieces, hipStream_t st);
void launch_frag_rows(const void *pieces, void *sums, uint32_t npieces, hipStream_t st);
void launch_frag_spread(const void *pieces, void *sums, uint32_t npieces, hipStream_t st);
void launch_frag_compare_rows(const void *pieces, void *sums, void *firsts, uint32_t npieces, hipStream_t st);
void launch_frag_fold(const void *frags, const void *sums, void *out, uint32_t nfrags, hipStream_t st);
void launch_frag_fold_diff(const void *frags, const void *sums, const void *firsts, void *out, uint32_t nfrags, hipStream_t st);
void launch_digest_leaves(const void *leaves, void *out, uint32_t nleaves, hipStream_t st);
void launch_digest_roots(const void *frags, const void *leaves, void *out, const void *expect, void *differs, uint32_t nfrags, hipStream_t st);
void launch_block_table(const void *jobs, uint32_t njobs, void *scratch, void *res, void *sizes, hipStream_t st);
void launch_move_extents(const void *chunks, uint32_t nchunks, void *buf, uint64_t cap, void *state, size_t state_bytes, hipStream_t st);

#define HIP_OK(x) ((x) == hipSuccess)

namespace csa {

constexpr uint32_t kMagicNum = 0x20130331u;          // csarc.cpp:283,593
constexpr uint64_t kHeaderSize = 24;                 // csarc.cpp:561
constexpr uint64_t kBlockCap = 1048576;              // csa_io.h:158
constexpr int kMaxStreams = 2048;        // = kMaxBatch of csc_host.cpp: one launch takes them all; the GPU starts the next workgroup where one ends
constexpr int kStageBufs = 8;
constexpr uint32_t kMaxFrags = CSA_MAX_FRAGMENTS;
constexpr const char *kDummyName = "****";           // csa_common.h:79

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---------------------------------------------------------------------------------------------
// index model -- csa_typedef.h:12-90
// ---------------------------------------------------------------------------------------------
struct Entry {
    int64_t edate = 0, esize = 0, eattr = 0;
    char ext[4] = {0, 0, 0, 0};
    std::vector<CSAFrag> frags;
    uint32_t row = 0;              // CSAMI_DeviceWrite: the entry's row in the caller's table
};
typedef std::map<std::string, Entry> Index;

struct FilePiece {                 // FileBlock: one file (or slice of it) inside a task
    std::string path;
    Index::iterator it;
    uint32_t checksum = 0;
    uint64_t off = 0, size = 0, posblock = 0;
};
struct Task {
    uint64_t total = 0;
    std::vector<FilePiece> files;
    uint32_t ab_id = 0;
    void add(const std::string &path, uint64_t off, uint64_t size, uint64_t posblock, uint32_t checksum, Index::iterator it)
    {
        FilePiece p;
        p.path = path; p.off = off; p.size = size; p.posblock = posblock; p.checksum = checksum; p.it = it;
        files.push_back(p);
        total += size;
    }
};
struct Extent { uint64_t off, size; };
typedef std::map<uint64_t, std::vector<Extent>> BlockIndex;

// ---------------------------------------------------------------------------------------------
// little-endian fields -- csa_indexpack.cpp:5-66
// ---------------------------------------------------------------------------------------------
inline void put_le(std::vector<uint8_t> &v, uint64_t x, int n) { for (int i = 0; i < n; i++) v.push_back((uint8_t)(x >> (8 * i))); }
inline void store_le(uint8_t *p, uint64_t x, int n) { for (int i = 0; i < n; i++) p[i] = (uint8_t)(x >> (8 * i)); }
inline uint64_t load_le(const uint8_t *p, int n) { uint64_t x = 0; for (int i = n - 1; i >= 0; i--) x = (x << 8) | p[i]; return x; }

std::vector<uint8_t> pack_index(const Index &index, const BlockIndex &abindex, const std::string &arcname);
bool unpack_index(Index &index, BlockIndex &abindex, const uint8_t *buf, uint64_t size);

// check_header, csarc.cpp:577-598
inline bool header_ok(const uint8_t *h)
{
    return h[0] == 'C' && h[1] == 'S' && h[2] == 'A' && h[7] == '1' && (uint32_t)load_le(h + 3, 4) == kMagicNum;
}

bool path_match(const char *a, const char *b);

struct Selection {
    std::vector<std::string> names;
    bool has(const char *name) const
    {
        if (names.empty()) return true;
        for (const std::string &f : names) if (path_match(f.c_str(), name)) return true;
        return false;
    }
};

inline Selection make_selection(const char *const *names, int n)
{
    Selection s;
    for (int i = 0; i < n; i++) s.names.push_back(names[i]);
    return s;
}

// ---- pieces of Add shared by the one-process path, the sharded (one process per GPU) path and the device-resident write ----
struct AddPlan {
    CSAOptions o;
    Index index;
    std::vector<Task> tasks;
};

// the tasks of P.index under P.o, whoever filled the index: the directory scan (plan_add) or the caller's table (plan_write)
int plan_index(AddPlan &P);

}   // namespace csa
