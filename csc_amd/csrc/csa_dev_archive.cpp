// csa_dev_archive.cpp -- the device-resident archive paths (C ABI in include/csa_mi355x.h): a `.csa` in HBM to file bytes in HBM
// and back.  The container format and the plan of an Add are csa_archive.cpp's (csa_internal.h); the kernels are
// csa_dev_kernels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "csa_internal.h"
#include "csa_waves.h"
#include "csa_dev_read.h"
#include "csa_dev_write.h"
#include "csa_dev_digest.h"
#include "csa_dev_move.h"

using namespace csa;

// ---------------------------------------------------------------------------------------------
// device-resident read: CSAMI_DeviceOpen / Plan / Read / Close, CSAMI_PlanDeviceLayout (include/csa_mi355x.h).
// Host side: the index, the layout of dst, the validation of everything the index says, the piece tables.  The bytes move in
// csa_dev_kernels.hip (tables and copy: csa_dev_read.h) and in CSCMI_DecodeDeviceBatch; CSAMI_DeviceReadStop is the same body with
// every task stopped behind its last selected byte (CSCMI_DecodeDeviceBatchStop).  All of them are one path over a device pointer
// per entry (ReadBufs, dev_read_run): CSAMI_DeviceReadInto hands the caller's pointers in, CSAMI_DeviceRead / ReadStop the layout's
// offsets into dst, and CSAMI_DeviceCompare the caller's pointers to be compared with instead of stored to.  CSAMI_DeviceReadSlices
// is that path over a layout that holds only the fragments its slices touch (dev_layout), with k_frag_slices as the middle kernel.
// The caller's side of an entry is a slice of a buffer (CSAMI_DeviceReadIntoSlices, CSAMI_DeviceCompareSlices; a whole buffer in the
// other calls): a wave in which a piece's side is the runs of a periodic pattern runs k_frag_spread / k_frag_compare_rows.
// ---------------------------------------------------------------------------------------------
struct CSADevArchive {
    const uint8_t *arc = nullptr;
    uint64_t arc_size = 0;
    Index index;
    BlockIndex abindex;
    std::map<uint64_t, uint64_t> task_raw;     // bid -> raw size
    uint64_t open_readback = 0;
    double kernel_ms[3] = {0, 0, 0};
};

namespace {

bool add_ok(uint64_t a, uint64_t b, uint64_t *out) { return !__builtin_add_overflow(a, b, out); }

csadev::Slice dev_slice(const CSADevSlice &s) { return csadev::Slice{s.offset, s.run, s.stride, s.count}; }

// "every byte of a buffer of n bytes": one run of n, nothing where n == 0
csadev::Slice whole_slice(uint64_t n) { return n ? csadev::Slice{0, n, n, 1} : csadev::Slice{0, 0, 0, 0}; }

// what a task of `raw` bytes' decoder holds: the dictionary (bounded by the raw size and by 1 GiB) and ~24 MiB of rings and buffers,
// as read_archive reckons
uint64_t decoder_need(uint64_t raw) { return std::min<uint64_t>(std::max<uint64_t>(raw, 1u << 20), 1ull << 30) + (24ull << 20); }

struct DevFilePlan { Index::const_iterator it; uint64_t offset, size; };
struct DevFrag { uint32_t file; uint32_t checksum; uint64_t posblock, size, posfile, idx; };   // idx: its place in the index, all fragments counted
struct DevTask { uint64_t bid = 0, total = 0, raw = 0, stop = 0; std::vector<DevFrag> frags; };   // stop: max(posblock + size) over `frags`, <= raw
struct DevLayout {
    std::vector<DevFilePlan> files;
    std::vector<DevTask> tasks;                // decode order
    uint64_t dst_bytes = 0;
    // CSAMI_DeviceReadSlices only: per entry its checked slice and the bytes it selects; the tasks then hold the TOUCHED fragments
    bool sliced = false;
    std::vector<csadev::Slice> slices;
    std::vector<uint64_t> slice_bytes;
    uint64_t touched_frags = 0, touched_bytes = 0;
    // CSAMI_DeviceReadDigests: the index's fragments, and which of the selected ones are empty (no task holds those)
    uint64_t index_frags = 0;
    std::vector<std::pair<uint64_t, uint32_t>> empty_idx;      // (place in the index, entry)
};

// A task's raw size: max(posblock + size) over ALL fragments of its bid.  false if any sum of the index wraps.
bool dev_task_sizes(const Index &index, std::map<uint64_t, uint64_t> &raw)
{
    raw.clear();
    for (const auto &kv : index)
        for (const CSAFrag &f : kv.second.frags) {
            uint64_t end, fend;
            if (!add_ok(f.posblock, f.size, &end) || !add_ok(f.posfile, f.size, &fend)) return false;
            uint64_t &r = raw[f.bid];
            r = std::max(r, end);
        }
    return true;
}

// The layout of dst and the tasks to decode for a selection.  false if the sum wraps.
// With `slices` (one per selected entry, nslices of them; false for another number and for a slice slice_check refuses) a fragment
// counts only if its entry's slice touches it: for the tasks, their order and their stops.
bool dev_layout(const Index &index, const std::map<uint64_t, uint64_t> &raw, const Selection &sel, DevLayout &L,
                const CSADevSlice *slices = nullptr, size_t nslices = 0)
{
    std::map<uint64_t, size_t> idmap;
    uint64_t off = 0;
    L.sliced = slices != nullptr;
    for (Index::const_iterator it = index.begin(); it != index.end(); ++it) {
        uint64_t idx = L.index_frags;
        L.index_frags += it->second.frags.size();
        if (!sel.has(it->first.c_str())) continue;
        uint64_t size = 0;
        const uint32_t fi = (uint32_t)L.files.size();
        for (const CSAFrag &f : it->second.frags) size = std::max(size, f.posfile + f.size);   // (checked by dev_task_sizes)
        csadev::Slice sl = {0, 0, 0, 0};
        if (L.sliced) {
            if (fi >= nslices) return false;
            sl = dev_slice(slices[fi]);
            uint64_t bytes;
            if (!csadev::slice_check(sl, size, &bytes)) return false;
            L.slices.push_back(sl);
            L.slice_bytes.push_back(bytes);
        }
        for (const CSAFrag &f : it->second.frags) {
            const uint64_t at = idx++;
            if (!f.size) { L.empty_idx.push_back(std::make_pair(at, fi)); continue; }
            if (L.sliced) {
                if (csadev::slice_next(sl, f.posfile) >= f.posfile + f.size) continue;
                L.touched_frags++;
                if (!add_ok(L.touched_bytes, f.size, &L.touched_bytes)) return false;
            }
            auto m = idmap.find(f.bid);
            if (m == idmap.end()) {
                m = idmap.insert(std::make_pair((uint64_t)f.bid, L.tasks.size())).first;
                L.tasks.push_back(DevTask());
                L.tasks.back().bid = f.bid;
                L.tasks.back().raw = raw.at(f.bid);
            }
            DevTask &t = L.tasks[m->second];
            t.frags.push_back(DevFrag{fi, f.checksum, f.posblock, f.size, f.posfile, at});
            if (!add_ok(t.total, f.size, &t.total)) return false;
            t.stop = std::max(t.stop, f.posblock + f.size);               // (checked by dev_task_sizes)
        }
        L.files.push_back(DevFilePlan{it, off, size});
        uint64_t r;
        if (!add_ok(size, 15, &r) || !add_ok(off, r & ~15ull, &off)) return false;
    }
    if (L.sliced && L.files.size() != nslices) return false;
    L.dst_bytes = off;
    std::sort(L.tasks.begin(), L.tasks.end(), [](const DevTask &a, const DevTask &b) {                        // csarc.cpp:430
        return a.total != b.total ? a.total > b.total : a.bid < b.bid;
    });
    return true;
}

void dev_fill_files(const DevLayout &L, CSADevFile *files, uint32_t cap)
{
    for (size_t i = 0; files && i < L.files.size() && i < cap; i++) {
        const DevFilePlan &p = L.files[i];
        CSADevFile &f = files[i];
        f.name = p.it->first.c_str();
        f.esize = p.it->second.esize; f.edate = p.it->second.edate; f.eattr = p.it->second.eattr;
        f.offset = p.offset; f.size = p.size;
        f.nfrags = (uint32_t)p.it->second.frags.size(); f.failed_frags = 0;
    }
}

// AsyncArchiveReader (csa_io.h:466-542) over a buffer: the task's archive blocks, each clipped to the archive; the first one
// that is cut short ends the stream (ExtentSource: a short read is end of file).  false if the total wraps.
bool dev_stream_extents(const std::vector<Extent> &in, uint64_t arc_size, std::vector<Extent> &out, uint64_t &total)
{
    out.clear();
    total = 0;
    for (const Extent &x : in) {
        const uint64_t avail = x.off < arc_size ? std::min<uint64_t>(x.size, arc_size - x.off) : 0;
        if (avail) {
            out.push_back(Extent{x.off, avail});
            if (!add_ok(total, avail, &total)) return false;
        }
        if (avail < x.size) break;
    }
    return true;
}

struct DevBuf {                                // device memory released at scope end
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    bool alloc(uint64_t n) { return n <= (uint64_t)SIZE_MAX && HIP_OK(hipMalloc(&p, (size_t)std::max<uint64_t>(n, 16))); }
    bool upload(const void *src, uint64_t n) { return alloc(n) && (!n || HIP_OK(hipMemcpy(p, src, (size_t)n, hipMemcpyHostToDevice))); }
};

struct DevTimer {                              // HIP-event time of this layer's three launches, by kernel
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    bool ok = false;
    DevTimer() { ok = HIP_OK(hipEventCreate(&ev[0])) && HIP_OK(hipEventCreate(&ev[1])); }
    ~DevTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    void begin() { (void)hipEventRecord(ev[0], st); }
    bool end(double *ms)                       // waits for the launch
    {
        float f = 0;
        if (!HIP_OK(hipGetLastError()) || !HIP_OK(hipEventRecord(ev[1], st)) || !HIP_OK(hipEventSynchronize(ev[1]))) return false;
        if (HIP_OK(hipEventElapsedTime(&f, ev[0], ev[1]))) *ms += f;
        return true;
    }
    // one launch (launch(): one of the launch_* calls on `st`), counted and waited for, its time added to *ms
    template <class F> bool timed(double *ms, uint64_t &launches, F launch)
    {
        begin();
        launch();
        launches++;
        return end(ms);
    }
};

// Where a launch is accounted: the HIP-event time of a piece pass and of a fold, and the caller's launch counter.
struct LaunchSlot { DevTimer &tm; double *ms, *ms_fold; uint64_t &launches; };

// The piece and fold tables for the fragments of a wave, their device copies and their launches.  A table holds one kind of leading
// pieces -- kSliced: SlicePieces (add_sliced); kSpread: SpreadPieces (add_spread); kGathered: GatherPieces (add_gathered), with
// pieces that are only summed behind them (add_summed) -- and runs itself: sum() the store / sum pass and k_frag_fold, compare()
// the compare pass and k_frag_fold_diff.  A table none of whose pieces is periodic goes through k_frag_pieces / k_frag_compare as the
// CopyPieces its pieces then are.  This is where a new kind of piece plugs in: a vector, an add_*, a line in lead() and in sum() or compare().
struct FragTables {
    enum Kind { kSliced, kSpread, kGathered };
    explicit FragTables(Kind k) : kind(k) {}
    std::vector<csadev::FragFold> frags;
    size_t summed() const { return pieces.size(); }        // the pieces add_summed made

    // CSAMI_DeviceReadSlices: the fragment of `size` > 0 bytes at src lies at [posfile, posfile + size) of an entry under the (checked)
    // slice sl, and dst is the entry's packed destination, or NULL.  Each 16 KiB cell is classified (slice_reduce).
    // false (here and below): more pieces than a launch takes.
    bool add_sliced(const uint8_t *src, uint8_t *dst, const csadev::Slice &sl, uint64_t posfile, uint64_t size, uint32_t checksum,
                    CSADevSliceStats &SL)
    {
        using namespace csadev;
        if (!add_frag(spieces.size(), size, checksum)) return false;
        piece_split(src, nullptr, size, kFragPiece, [&](uint64_t k, const CopyPiece &p) {
            SlicePiece sp = {p.src, nullptr, p.len, 0, 0, 0, 0, 0};
            SliceCut c;
            const SliceKind kd = dst ? slice_reduce(sl, posfile + k * kFragPiece, p.len, c) : kSliceNone;
            if (kd != kSliceNone) sp.dst = (uint8_t *)((uintptr_t)dst + c.dst);
            if (kd == kSlicePeriodic) { sp.lo = c.lo; sp.hi = c.hi; sp.phase = c.phase; sp.run = c.run; sp.stride = c.stride; }
            (kd == kSlicePeriodic ? SL.periodic_pieces : SL.plain_pieces)++;
            spieces.push_back(sp);
        });
        return true;
    }
    // CSAMI_DeviceWriteSlices: a fragment of `size` > 0 bytes that is the packed bytes [at, at + size) of the (checked) slice sl of the
    // buffer `buf`, gathered to dst.  Its pieces and their sums come first: add_summed counts from behind them.  dst == NULL
    // (CSAMI_DeviceUpdate's check under CSAMI_UPDATE_TRUST_SUMS): the fragment is summed where it lies and folded against `checksum`.
    bool add_gathered(const uint8_t *buf, uint8_t *dst, const csadev::Slice &sl, uint64_t at, uint64_t size, CSADevGatherStats &G,
                      uint32_t checksum = 0)
    {
        stores = stores || dst;
        return pieces.empty() && add_rows(gpieces, buf, sl, at, size, size, checksum, G.plain_pieces, G.periodic_pieces,
                                          [&](uint64_t off, uint32_t len, uint32_t, const uint8_t *side) {
            return csadev::GatherPiece{side, dst ? dst + off : nullptr, 0, len, 0, 0, 0, nullptr, nullptr};
        });
    }
    // behind the gathered fragments: a fragment of `size` > 0 bytes that is summed where it lies, at src
    bool add_summed(const uint8_t *src, uint64_t size)
    {
        using namespace csadev;
        if (!add_frag(gpieces.size() + pieces.size(), size, 0)) return false;
        piece_split(src, nullptr, size, kFragPiece, [&](uint64_t, const CopyPiece &p) { pieces.push_back(p); });
        return true;
    }
    // The read paths over the caller's buffers: the fragment's delivered bytes, at src, are the packed bytes [posfile, posfile + size)
    // of its entry, whose side in the caller's buffer `buf` (NULL: none) is what the (checked) slice sl selects of it.  The leading
    // `use` <= size bytes have that side -- all of them where they are stored, the compared ones with `compare` -- and the rest is
    // summed only.
    bool add_spread(const uint8_t *src, uint8_t *buf, const csadev::Slice &sl, uint64_t posfile, uint64_t size, uint32_t checksum,
                    uint64_t use, bool compare, CSADevSpreadStats &X)
    {
        stores = stores || buf;
        return add_rows(xpieces, buf, sl, posfile, size, buf ? use : 0, checksum, X.plain_pieces, X.periodic_pieces,
                        [&](uint64_t off, uint32_t len, uint32_t u, const uint8_t *side) {
            return csadev::SpreadPiece{src + off, (uint8_t *)side, 0, len, 0, 0, compare ? u : 0, nullptr, nullptr};
        });
    }

    // The store / sum pass over the leading pieces (`always`: even where there is none -- a read wave and a check wave are always the
    // same three launches), the sum pass over the pieces behind them where there are any, and the fold: res[i] is fragment i's.
    // *uploaded (NULL: not counted) gets the bytes of the tables.
    bool sum(const LaunchSlot &at, bool always, uint64_t *uploaded, std::vector<csadev::FragResult> &res)
    {
        using namespace csadev;
        const uint32_t nlead = (uint32_t)lead().n, nsum = (uint32_t)pieces.size();
        const bool rows = plan_rows();
        if (!upload<FragResult>(rows, uploaded)) return false;
        if ((always || nlead) && !at.tm.timed(at.ms, at.launches, [&] {
                if (kind == kSliced) launch_frag_slices(d_lead.p, d_sums.p, nlead, at.tm.st);
                else if (!rows) launch_frag_pieces(d_pieces.p, d_sums.p, nlead, stores, at.tm.st);
                else if (kind == kSpread) launch_frag_spread(d_lead.p, d_sums.p, nlead, at.tm.st);
                else launch_frag_rows(d_lead.p, d_sums.p, nlead, at.tm.st); })) return false;
        // (the summed pieces lie behind the leading ones in d_pieces where those became CopyPieces, else at its front)
        if (nsum && !at.tm.timed(at.ms, at.launches, [&] {
                launch_frag_pieces((const CopyPiece *)d_pieces.p + (rows ? 0 : nlead), (PieceSums *)d_sums.p + nlead, nsum, false, at.tm.st); }))
            return false;
        return fold(at, res);
    }
    // The compare pass over a kSpread table -- each piece's leading cmp bytes against the caller's -- and the fold: res[i].first is the
    // first differing offset in fragment i, its size if there is none.
    bool compare(const LaunchSlot &at, uint64_t *uploaded, std::vector<csadev::FragDiff> &res)
    {
        const uint32_t n = (uint32_t)xpieces.size();
        const bool rows = plan_rows();
        if (!upload<csadev::FragDiff>(rows, uploaded)) return false;
        if (!at.tm.timed(at.ms, at.launches, [&] {
                if (rows) launch_frag_compare_rows(d_lead.p, d_sums.p, d_firsts.p, n, at.tm.st);
                else launch_frag_compare(d_pieces.p, d_sums.p, d_firsts.p, n, at.tm.st); })) return false;
        return fold(at, res);
    }

private:
    const Kind kind;
    std::vector<csadev::SlicePiece> spieces;
    std::vector<csadev::GatherPiece> gpieces;
    std::vector<csadev::SpreadPiece> xpieces;
    std::vector<csadev::CopyPiece> pieces;
    uint64_t periodic = 0;                     // leading pieces that cross a run border
    bool stores = false;                       // a leading piece has a side it is stored to
    DevBuf d_lead, d_pieces, d_frags, d_sums, d_res, d_firsts;
    struct Lead { const void *p; size_t n, bytes; };
    Lead lead() const
    {
        return kind == kSliced   ? Lead{spieces.data(), spieces.size(), spieces.size() * sizeof(csadev::SlicePiece)}
               : kind == kSpread ? Lead{xpieces.data(), xpieces.size(), xpieces.size() * sizeof(csadev::SpreadPiece)}
                                 : Lead{gpieces.data(), gpieces.size(), gpieces.size() * sizeof(csadev::GatherPiece)};
    }
    bool add_frag(size_t first, uint64_t size, uint32_t checksum)
    {
        const uint64_t np = csadev::piece_count(size, csadev::kFragPiece);
        if (first + np > 0x7FFFFFFFull) return false;
        frags.push_back(csadev::FragFold{size, (uint32_t)first, (uint32_t)np, checksum, 0});
        return true;
    }
    // The row planner of add_gathered and add_spread: the fragment is the packed bytes [at, at + size) of the slice sl of `buf`, and
    // the leading `use` bytes of it have that side.  Each 16 KiB cell is planned by gather_reduce: make(off, len, u, side) gives the
    // piece of the cell at `off` whose leading u bytes have the one contiguous side `side` (NULL where u == 0); a cell that crosses a
    // run border gets its period and the slice's hull on top, and counts as periodic.
    template <class Piece, class Make>
    bool add_rows(std::vector<Piece> &out, const uint8_t *buf, const csadev::Slice &sl, uint64_t at, uint64_t size, uint64_t use, uint32_t checksum,
                  uint64_t &n_plain, uint64_t &n_periodic, Make make)
    {
        using namespace csadev;
        if (!add_frag(out.size(), size, checksum)) return false;
        const uint8_t *lo = use ? buf + sl.offset : nullptr, *hi = use ? lo + (sl.count - 1) * sl.stride + sl.run : nullptr;
        for (uint64_t off = 0; off < size; off += kFragPiece) {
            const uint32_t len = (uint32_t)std::min<uint64_t>(size - off, kFragPiece);
            const uint32_t u = (uint32_t)(use > off ? std::min<uint64_t>(use - off, len) : 0);
            GatherCut c = {0, 0, 0, 0};
            const bool whole = !u || gather_reduce(sl, at + off, u, c);
            Piece p = make(off, len, u, u ? buf + c.src : nullptr);
            if (!whole) { p.stride = c.stride; p.phase = c.phase; p.run = c.run; p.lo = lo; p.hi = hi; periodic++; }
            (whole ? n_plain : n_periodic)++;
            out.push_back(p);
        }
        return true;
    }
    static uint32_t cmp_of(const csadev::GatherPiece &) { return 0; }
    static uint32_t cmp_of(const csadev::SpreadPiece &x) { return x.cmp; }
    template <class Piece> void as_plain(std::vector<Piece> &rows)
    {
        std::vector<csadev::CopyPiece> front;
        front.reserve(rows.size() + pieces.size());
        for (const Piece &r : rows) front.push_back(csadev::CopyPiece{r.src, r.dst, r.len, cmp_of(r)});
        front.insert(front.end(), pieces.begin(), pieces.end());
        pieces.swap(front);
        rows.clear();
    }
    // true: the leading pieces go through their own kernel.  false: none of them is periodic, and they have become the CopyPieces they
    // are, in front of `pieces`.
    bool plan_rows()
    {
        if (kind == kSliced || periodic) return true;
        if (kind == kSpread) as_plain(xpieces); else as_plain(gpieces);
        return false;
    }
    // the tables to the device, and room for the sums and for a result of type R per fragment
    template <class R> bool upload(bool rows, uint64_t *uploaded)
    {
        const Lead ld = lead();
        const size_t np = ld.n + pieces.size();
        if (uploaded) *uploaded += ld.bytes + pieces.size() * sizeof(csadev::CopyPiece) + frags.size() * sizeof(csadev::FragFold);
        return (!rows || d_lead.upload(ld.p, ld.bytes))
               && ((rows && kind != kGathered) || d_pieces.upload(pieces.data(), pieces.size() * sizeof(csadev::CopyPiece)))
               && d_frags.upload(frags.data(), frags.size() * sizeof(csadev::FragFold))
               && d_sums.alloc(np * sizeof(csadev::PieceSums))
               && d_res.alloc(frags.size() * sizeof(R))
               && (!std::is_same<R, csadev::FragDiff>::value || d_firsts.alloc(np * sizeof(uint32_t)));
    }
    // k_frag_fold over the sums the piece pass left (k_frag_fold_diff: and over the first differences), and the fragments' results
    // read back: res.size() * sizeof(R) bytes
    template <class R> bool fold(const LaunchSlot &at, std::vector<R> &res)
    {
        const uint32_t n = (uint32_t)frags.size();
        if (!at.tm.timed(at.ms_fold, at.launches, [&] {
                if (std::is_same<R, csadev::FragDiff>::value) launch_frag_fold_diff(d_frags.p, d_sums.p, d_firsts.p, d_res.p, n, at.tm.st);
                else launch_frag_fold(d_frags.p, d_sums.p, d_res.p, n, at.tm.st); })) return false;
        res.resize(n);
        return res.empty() || HIP_OK(hipMemcpy(res.data(), d_res.p, res.size() * sizeof(R), hipMemcpyDeviceToHost));
    }
};

thread_local double g_digest_ms[2] = {0, 0};         // CSAMI_DeviceDigestKernelMs

// One digest pass (csa_dev_digest.h): the leaf and fragment tables of the fragments added, their device copies and their two launches
// -- k_digest_leaves, one lane per 16 KiB leaf, and k_digest_roots, one lane per fragment, which stores fragment i's digest to
// out[frags[i].out] and compares it with expect[frags[i].expect] -- and one word per fragment read back.
struct DigestPass {
    std::vector<csadev::DigestLeaf> leaves;
    std::vector<csadev::DigestFrag> frags;
    uint64_t bytes = 0;
    // a fragment of `size` bytes that is the packed bytes [at, at + size) of the (checked) slice sl of the buffer `buf`; size == 0:
    // the empty fragment, nothing of buf or sl is looked at.  false: more leaves than a launch takes.
    bool add(const uint8_t *buf, const csadev::Slice &sl, uint64_t at, uint64_t size, uint64_t out, uint64_t expect)
    {
        const uint64_t first = leaves.size(), n = std::max<uint64_t>(csadev::piece_count(size, csadev::kDigestLeaf), 1);
        if (first + n > 0x7FFFFFFFull || frags.size() >= 0x7FFFFFFFull) return false;
        csadev::digest_split(buf, sl, at, size, [&](const csadev::DigestLeaf &l) { leaves.push_back(l); });
        frags.push_back(csadev::DigestFrag{out, expect, (uint32_t)first, (uint32_t)n});
        bytes += size;
        return true;
    }
    // a fragment that lies at src, contiguous
    bool add(const uint8_t *src, uint64_t size, uint64_t out, uint64_t expect)
    {
        return add(src, csadev::Slice{0, size, size, size ? 1u : 0u}, 0, size, out, expect);
    }
    // differs[i]: 1 where fragment i was compared and its digest is not the expected one.  ds is added to.  (The tables' bytes are
    // in no statistic: the write's upload_bytes stays what it is without a digest table.)
    bool run(DevTimer &tm, CSADevDigest *out, const CSADevDigest *expect, CSADevDigestStats &ds, std::vector<uint32_t> &differs)
    {
        differs.assign(frags.size(), 0);
        if (frags.empty()) return true;
        const uint32_t nl = (uint32_t)leaves.size(), nf = (uint32_t)frags.size();
        DevBuf d_leaves, d_frags, d_dig, d_diff;
        if (!d_leaves.upload(leaves.data(), nl * sizeof(csadev::DigestLeaf)) || !d_frags.upload(frags.data(), nf * sizeof(csadev::DigestFrag))
            || !d_dig.alloc((uint64_t)nl * sizeof(csadev::DigestWords)) || !d_diff.alloc(nf * sizeof(uint32_t))) return false;
        double ms[2] = {0, 0};
        if (!tm.timed(&ms[0], ds.launches, [&] { launch_digest_leaves(d_leaves.p, d_dig.p, nl, tm.st); })
            || !tm.timed(&ms[1], ds.launches, [&] { launch_digest_roots(d_frags.p, d_dig.p, out, expect, d_diff.p, nf, tm.st); })
            || !HIP_OK(hipMemcpy(differs.data(), d_diff.p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost))) return false;
        g_digest_ms[0] += ms[0]; g_digest_ms[1] += ms[1];
        ds.kernel_ms += ms[0] + ms[1];
        ds.frags += nf; ds.leaves += nl; ds.digested_bytes += bytes;
        for (uint32_t i = 0; i < nf; i++)
            if (differs[i]) { ds.mismatches++; ds.first_mismatch = std::min<uint64_t>(ds.first_mismatch, frags[i].out); }
        return true;
    }
};

// what a call that digests hands down: the two tables (either may be NULL) and its statistics
struct DigestCall { CSADevDigest *out; const CSADevDigest *expect; CSADevDigestStats ds; };

bool ranges_meet(const void *a, uint64_t an, const void *b, uint64_t bn)
{
    const uint64_t a0 = (uint64_t)(uintptr_t)a, b0 = (uint64_t)(uintptr_t)b;
    return an && bn && a && b && a0 <= b0 + (bn - 1) && b0 <= a0 + (an - 1);
}

// The coded streams of a wave's tasks, staged for CSCMI_DecodeDeviceBatch (csa_worker.cpp:59-90 for every task at once): one
// k_gather_extents launch brings every task's 10 property bytes -- they may span archive blocks -- into a 16-byte slot, and the stream
// of every task of more than one archive block into one piece of d_gat; a stream of one block is decoded where it lies.  The
// property bytes are read back.  Both directions use it: the read for the tasks it decodes, the update for the candidates it checks.
struct StagedStreams {
    // a task's archive blocks clipped to the archive (dev_stream_extents), their bytes, and the room its decoded bytes get
    struct Task { const std::vector<Extent> *ext; uint64_t stream, cap; };
    std::vector<Task> tasks;
    std::vector<uint8_t> props;                // 16 bytes per task, the first CSC_PROP_SIZE of them read back
    uint64_t raw_bytes = 0;                    // all the decoded bytes' room
    uint64_t table_bytes = 0;                  // the piece table of the gather, as uploaded

    // body == false: the property bytes only -- no stream is gathered, nothing will be decoded.  The launch is `launches`' and its
    // time *ms's.  false: a device error, or sizes that wrap.
    bool stage(const uint8_t *arc_, bool body, DevTimer &tm, double *ms, uint64_t &launches)
    {
        using namespace csadev;
        const size_t count = tasks.size();
        arc = arc_;
        gat_off.assign(count, 0);
        raw_off.assign(count, 0);
        uint64_t gat_bytes = 0, r;
        for (size_t k = 0; k < count && body; k++) {
            const Task &t = tasks[k];
            if (t.stream > CSC_PROP_SIZE && t.ext->size() > 1) {
                gat_off[k] = gat_bytes;
                if (!add_ok(t.stream - CSC_PROP_SIZE, 255, &r) || !add_ok(gat_bytes, r & ~255ull, &gat_bytes)) return false;
            }
            raw_off[k] = raw_bytes;
            if (!add_ok(t.cap, 255, &r) || !add_ok(raw_bytes, r & ~255ull, &raw_bytes)) return false;
        }
        if (!d_gat.alloc(gat_bytes) || !d_raw.alloc(raw_bytes) || !d_props.alloc(16 * count)) return false;
        std::vector<CopyPiece> gp;
        for (size_t k = 0; k < count; k++) {
            uint64_t pos = 0;                                                    // position in the task's stream
            for (const Extent &x : *tasks[k].ext) {
                const uint8_t *src = arc + x.off;
                uint64_t n = x.size;
                if (pos < CSC_PROP_SIZE) {
                    const uint64_t h = std::min<uint64_t>(CSC_PROP_SIZE - pos, n);
                    gp.push_back(CopyPiece{src, (uint8_t *)d_props.p + 16 * k + pos, (uint32_t)h, 0});
                    src += h; n -= h; pos += h;
                }
                if (body && tasks[k].ext->size() > 1 && n)
                    piece_split(src, (uint8_t *)d_gat.p + gat_off[k] + (pos - CSC_PROP_SIZE), n, kGatherPiece,
                                [&](uint64_t, const CopyPiece &p) { gp.push_back(p); });
                pos += n;
                if (!body && pos >= CSC_PROP_SIZE) break;
            }
        }
        if (gp.size() > 0x7FFFFFFFull) return false;
        props.assign(16 * count, 0);
        table_bytes = gp.size() * sizeof(CopyPiece);
        DevBuf d_gp;
        return d_gp.upload(gp.data(), table_bytes)
               && tm.timed(ms, launches, [&] { launch_gather_extents(d_gp.p, (uint32_t)gp.size(), tm.st); })
               && HIP_OK(hipMemcpy(props.data(), d_props.p, props.size(), hipMemcpyDeviceToHost));
    }
    bool has_props(size_t k) const { return tasks[k].stream >= CSC_PROP_SIZE; }       // csa_worker.cpp:77-80: no property bytes, no decoder
    const uint8_t *props_of(size_t k) const { return props.data() + 16 * k; }
    const uint8_t *raw(size_t k) const { return (const uint8_t *)d_raw.p + raw_off[k]; }   // where task k's decoded bytes go
    // the decode of task k (has_props(k), staged with its body): its properties, its stream behind them, its room
    CSCMIDevDecode job(size_t k) const
    {
        const Task &t = tasks[k];
        CSCMIDevDecode j;
        memset(&j, 0, sizeof(j));
        CSCDec_ReadProperties(&j.props, const_cast<uint8_t *>(props_of(k)));
        j.src = t.ext->size() > 1 ? (const uint8_t *)d_gat.p + gat_off[k] : arc + (*t.ext)[0].off + CSC_PROP_SIZE;
        j.src_size = (size_t)(t.stream - CSC_PROP_SIZE);
        j.dst = (uint8_t *)d_raw.p + raw_off[k];
        j.dst_cap = (size_t)t.cap;
        return j;
    }

private:
    const uint8_t *arc = nullptr;
    DevBuf d_gat, d_raw, d_props;
    std::vector<uint64_t> gat_off, raw_off;
};

// The caller's side of a read: entry i of the layout (L.files) is delivered to -- or, with `diffs`, compared with -- ptrs[i].
struct ReadBufs {
    uint8_t *const *ptrs = nullptr;            // per entry; NULL (the table, or an entry of it): verified only
    const uint64_t *lim = nullptr;             // compare: per entry, the bytes that are compared -- min(the entry's size, the caller's)
    CSADevDiff *diffs = nullptr;               // compare: per entry; first_diff, CSA_DIFF_BYTES and CSA_DIFF_SHORT are added here
    CSADevSliceStats *slice_stats = nullptr;   // slices (a layout with L.sliced, never null there): ptrs[i] takes entry i's packed slice, and the piece counts are added here
    const csadev::Slice *bslices = nullptr;    // per entry, checked: what of the caller's buffer ptrs[i][0, bsizes[i]) is the entry's side -- the packed bytes it
    const uint64_t *bsizes = nullptr;          // selects take the entry (a layout with L.sliced: its packed slice); count 0: nothing, as where ptrs[i] is NULL
    CSADevSpreadStats *spread = nullptr;       // never null without L.sliced: the piece counts are added here
    DigestCall *dg = nullptr;                  // CSAMI_DeviceReadDigests: every delivered fragment is also digested, and compared where dg->expect is given
    uint8_t *at(uint32_t file) const { return ptrs ? ptrs[file] : nullptr; }
};

// One wave: tasks [first, first + count) of L.  Returns 0, -1 (a stream failed) or CSCMI_DEVICE_ERROR.
// SS != nullptr (CSAMI_DeviceReadStop): a task is decoded only up to its `stop` -- capacity, scratch and stop position are that --
// and SS is added to.  The coded stream of a task of several archive blocks is still gathered whole: how many coded bytes a
// prefix of the raw bytes needs is not known before it is decoded.
int dev_read_wave(CSADevArchive &A, const DevLayout &L, size_t first, size_t count, const ReadBufs &B, std::vector<uint32_t> &failed,
                  CSADevReadStats &S, DevTimer &tm, CSADevStopStats *SS)
{
    using namespace csadev;
    static const std::vector<Extent> kNoBlocks;
    int worst = 0;
    // 1. the streams, staged: where each task's coded bytes lie, and its decoded bytes' room
    std::vector<std::vector<Extent>> ext(count);
    StagedStreams St;
    for (size_t k = 0; k < count; k++) {
        const DevTask &t = L.tasks[first + k];
        auto ab = A.abindex.find(t.bid);
        uint64_t total;
        if (!dev_stream_extents(ab == A.abindex.end() ? kNoBlocks : ab->second, A.arc_size, ext[k], total)) return CSCMI_DEVICE_ERROR;
        St.tasks.push_back(StagedStreams::Task{&ext[k], total, SS ? t.stop : t.raw});
    }
    if (!St.stage(A.arc, true, tm, &A.kernel_ms[0], S.launches)) return CSCMI_DEVICE_ERROR;
    S.readback_bytes += St.props.size();

    // 2. decode
    std::vector<CSCMIDevDecode> jobs;
    std::vector<size_t> job_task;
    std::vector<uint64_t> stops;
    std::vector<uint64_t> produced(count, 0);
    for (size_t k = 0; k < count; k++) {
        if (!St.has_props(k)) { worst = -1; continue; }
        jobs.push_back(St.job(k));
        job_task.push_back(k);
        stops.push_back(jobs.back().dst_cap);
    }
    if (SS) {
        SS->scratch_bytes += St.raw_bytes;
        for (size_t k = 0; k < count; k++) {
            const DevTask &t = L.tasks[first + k];
            SS->task_raw_bytes += t.raw;
            if (t.stop < t.raw) SS->stopped_tasks++;
        }
    }
    if (!jobs.empty()) {
        CSCMIDevDecodeStats ds;
        memset(&ds, 0, sizeof(ds));
        if ((SS ? CSCMI_DecodeDeviceBatchStop((int)jobs.size(), jobs.data(), stops.data(), NULL, &ds)
                : CSCMI_DecodeDeviceBatch((int)jobs.size(), jobs.data(), NULL, &ds)) != 0) return CSCMI_DEVICE_ERROR;
        S.decode_launches += ds.launches;
        for (size_t i = 0; i < jobs.size(); i++) {
            if (jobs[i].rc == CSCMI_DEVICE_ERROR) return CSCMI_DEVICE_ERROR;
            if (SS) SS->decoded_bytes += jobs[i].produced;
            if (jobs[i].rc != 0) worst = -1;                                   // (WRITE_ERROR: more than the raw size -- a decode error here)
            produced[job_task[i]] = std::min<uint64_t>(jobs[i].produced, jobs[i].dst_cap);   // a failed stream still delivered this much
        }
    }

    // 3. scatter (or compare) and verify: the fragments at least one byte of which was delivered, clipped to what was delivered
    // (both launches even when no fragment was delivered: a wave is always the same three)
    FragTables T(L.sliced ? FragTables::kSliced : FragTables::kSpread);
    std::vector<uint32_t> ff_file;
    std::vector<uint64_t> ff_posfile;
    DigestPass DP;
    for (size_t k = 0; k < count; k++) {
        const DevTask &t = L.tasks[first + k];
        for (const DevFrag &f : t.frags) {
            const uint64_t n = f.posblock < produced[k] ? std::min<uint64_t>(f.size, produced[k] - f.posblock) : 0;
            uint8_t *p = B.at(f.file);
            uint64_t cmp = 0;
            if (B.diffs && p && B.lim[f.file] > f.posfile) {
                const uint64_t want = std::min<uint64_t>(f.size, B.lim[f.file] - f.posfile);
                cmp = std::min(n, want);
                if (n < want) B.diffs[f.file].status |= CSA_DIFF_SHORT;
            }
            if (!n) continue;
            const uint8_t *src = St.raw(k) + f.posblock;
            if (!(L.sliced ? T.add_sliced(src, p, L.slices[f.file], f.posfile, n, f.checksum, *B.slice_stats)
                           : T.add_spread(src, p, B.bslices[f.file], f.posfile, n, f.checksum, B.diffs ? cmp : n, B.diffs != nullptr, *B.spread)))
                return CSCMI_DEVICE_ERROR;
            ff_file.push_back(f.file);
            ff_posfile.push_back(f.posfile);
            if (B.dg && !DP.add(src, n, f.idx, B.dg->expect ? f.idx : kDigestNone)) return CSCMI_DEVICE_ERROR;
        }
    }
    const LaunchSlot slot = {tm, &A.kernel_ms[1], &A.kernel_ms[2], S.launches};
    std::vector<FragResult> res;
    if (B.diffs) {
        std::vector<FragDiff> rd;
        if (!T.compare(slot, nullptr, rd)) return CSCMI_DEVICE_ERROR;
        S.readback_bytes += rd.size() * sizeof(FragDiff);
        for (size_t i = 0; i < rd.size(); i++) {
            res.push_back(FragResult{rd[i].adler, rd[i].ok});
            if (rd[i].first >= T.frags[i].size) continue;
            CSADevDiff &d = B.diffs[ff_file[i]];
            d.status |= CSA_DIFF_BYTES;
            d.first_diff = std::min(d.first_diff, ff_posfile[i] + rd[i].first);
        }
    } else {
        if (!T.sum(slot, true, nullptr, res)) return CSCMI_DEVICE_ERROR;
        S.readback_bytes += res.size() * sizeof(FragResult);
    }
    std::vector<uint32_t> differs(res.size(), 0);
    if (B.dg && !DP.run(tm, B.dg->out, B.dg->expect, B.dg->ds, differs)) return CSCMI_DEVICE_ERROR;
    if (B.dg) S.readback_bytes += differs.size() * sizeof(uint32_t);
    for (size_t i = 0; i < res.size(); i++)
        if (!res[i].ok || differs[i]) {
            fprintf(stderr, "******** %s extraction/verify failed\n", L.files[ff_file[i]].it->first.c_str());   // csa_io.h:332,398
            failed[ff_file[i]]++;
            S.verify_failures++;
        }
    return worst;
}

}   // namespace

extern "C" {

int CSAMI_DeviceOpen(const void *arc_dev, uint64_t arc_size, CSADevArchive **out)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    const uint8_t *arc = (const uint8_t *)arc_dev;
    uint8_t hdr[kHeaderSize];
    if (!arc || arc_size < kHeaderSize) { fprintf(stderr, "Invalid csarc file\n"); return 1; }
    if (!HIP_OK(hipMemcpy(hdr, arc, kHeaderSize, hipMemcpyDeviceToHost))) return CSCMI_DEVICE_ERROR;
    if (!header_ok(hdr)) { fprintf(stderr, "Invalid csarc file\n"); return 1; }
    const uint64_t index_pos = load_le(hdr + 8, 8);
    const uint32_t csize = (uint32_t)load_le(hdr + 16, 4), rsize = (uint32_t)load_le(hdr + 20, 4);
    if (index_pos > arc_size || csize > arc_size - index_pos || csize < CSC_PROP_SIZE) { fprintf(stderr, "Invalid csarc file\n"); return -1; }
    uint8_t ph[CSC_PROP_SIZE];
    if (!HIP_OK(hipMemcpy(ph, arc + index_pos, CSC_PROP_SIZE, hipMemcpyDeviceToHost))) return CSCMI_DEVICE_ERROR;
    std::vector<uint8_t> raw(rsize);
    {
        DevBuf d_raw;
        if (!d_raw.alloc(rsize)) return CSCMI_DEVICE_ERROR;
        CSCMIDevDecode j;
        memset(&j, 0, sizeof(j));
        CSCDec_ReadProperties(&j.props, ph);
        j.src = arc + index_pos + CSC_PROP_SIZE;
        j.src_size = csize - CSC_PROP_SIZE;
        j.dst = d_raw.p;
        j.dst_cap = rsize;
        if (CSCMI_DecodeDeviceBatch(1, &j, NULL, NULL) != 0 || j.rc == CSCMI_DEVICE_ERROR) return CSCMI_DEVICE_ERROR;
        if (j.rc != 0 || j.produced != rsize) { fprintf(stderr, "Invalid csarc file (index)\n"); return -1; }
        if (rsize && !HIP_OK(hipMemcpy(raw.data(), d_raw.p, rsize, hipMemcpyDeviceToHost))) return CSCMI_DEVICE_ERROR;
    }
    CSADevArchive *A = new CSADevArchive();
    A->arc = arc;
    A->arc_size = arc_size;
    A->open_readback = kHeaderSize + CSC_PROP_SIZE + rsize;
    if (!unpack_index(A->index, A->abindex, raw.data(), rsize) || !dev_task_sizes(A->index, A->task_raw)) {
        fprintf(stderr, "Invalid csarc file (index)\n");
        delete A;
        return -1;
    }
    *out = A;
    return 0;
}

int CSAMI_DevicePlan(CSADevArchive *a, const char *const *names, int nnames,
                     CSADevFile *files, uint32_t cap, uint32_t *n_files, uint64_t *dst_bytes)
{
    DevLayout L;
    if (!a || !dev_layout(a->index, a->task_raw, make_selection(names, nnames), L)) return -1;
    dev_fill_files(L, files, cap);
    if (n_files) *n_files = (uint32_t)L.files.size();
    if (dst_bytes) *dst_bytes = L.dst_bytes;
    return 0;
}

}   // extern "C"

namespace {

// false where CSAMI_CheckSlices refuses the caller's buffers: the slice B.bslices[i] of B.ptrs[i], nothing where that is NULL
bool dev_bufs_ok(const CSADevArchive *a, const DevLayout &L, const ReadBufs &B, bool disjoint)
{
    if (!B.ptrs) return true;
    std::vector<CSADevSlice> sl(L.files.size(), CSADevSlice{0, 0, 0, 0});
    for (size_t i = 0; i < L.files.size(); i++)
        if (B.ptrs[i]) sl[i] = CSADevSlice{B.bslices[i].offset, B.bslices[i].run, B.bslices[i].stride, B.bslices[i].count};
    return CSAMI_CheckSlices((const void *const *)B.ptrs, B.bsizes, sl.data(), (uint32_t)L.files.size(), a->arc, a->arc_size, disjoint, nullptr) == 0;
}

// The waves of a read over buffers dev_bufs_ok has passed.  ss: stop every task behind its last selected byte, and add to *ss.
// `failed` gets one count per entry.
int dev_read_run(CSADevArchive *a, const DevLayout &L, const ReadBufs &B, const CSAOptions *opt, std::vector<uint32_t> &failed,
                 CSADevReadStats &S, CSADevStopStats *ss)
{
    const double t0 = now_s();
    failed.assign(L.files.size(), 0);
    CSAOptions o;
    if (opt) o = *opt; else CSA_OptionsInit(&o);
    a->kernel_ms[0] = a->kernel_ms[1] = a->kernel_ms[2] = 0;

    size_t mem_free = 0, mem_total = 0;
    if (!HIP_OK(hipMemGetInfo(&mem_free, &mem_total))) return CSCMI_DEVICE_ERROR;
    const uint64_t budget = hbm_budget(o, mem_free);
    const size_t width = o.device_streams > 0 ? (size_t)o.device_streams : L.tasks.size();
    DevTimer tm;
    if (!tm.ok) return CSCMI_DEVICE_ERROR;
    int worst = 0;
    S.readback_bytes = a->open_readback;
    if (B.dg && !L.empty_idx.empty()) {                                       // the zero-size fragments: no task holds them
        DigestPass DP;
        std::vector<uint32_t> differs;
        for (const auto &e : L.empty_idx)
            if (!DP.add(nullptr, 0, e.first, B.dg->expect ? e.first : csadev::kDigestNone)) return CSCMI_DEVICE_ERROR;
        if (!DP.run(tm, B.dg->out, B.dg->expect, B.dg->ds, differs)) return CSCMI_DEVICE_ERROR;
        S.readback_bytes += differs.size() * sizeof(uint32_t);
        for (size_t i = 0; i < differs.size(); i++)
            if (differs[i]) {
                fprintf(stderr, "******** %s extraction/verify failed\n", L.files[L.empty_idx[i].second].it->first.c_str());
                failed[L.empty_idx[i].second]++;
                S.verify_failures++;
            }
    }
    for (size_t first = 0; first < L.tasks.size() && worst != CSCMI_DEVICE_ERROR;) {
        // the task's decoded bytes and (at most) a copy of its stream, plus what its decoder holds
        // (stopped early: the decoded bytes are `stop`; the dictionary and the stream's copy are what they were)
        const size_t count = wave_count(first, L.tasks.size(), width, budget, [&](size_t t) {
            const uint64_t raw = L.tasks[t].raw, out = ss ? L.tasks[t].stop : raw;
            uint64_t need = decoder_need(raw);
            if (!add_ok(need, out, &need) || !add_ok(need, raw, &need)) need = UINT64_MAX;
            return need;
        });
        int r = dev_read_wave(*a, L, first, count, B, failed, S, tm, ss);
        if (r < 0 && worst != CSCMI_DEVICE_ERROR) worst = r;
        S.waves++;
        for (size_t k = first; k < first + count; k++) { S.tasks++; S.frags += L.tasks[k].frags.size(); S.raw_bytes += L.tasks[k].total; }
        first += count;
    }
    S.kernel_ms = a->kernel_ms[0] + a->kernel_ms[1] + a->kernel_ms[2];
    S.seconds_total = now_s() - t0;
    if (worst == CSCMI_DEVICE_ERROR) return CSCMI_DEVICE_ERROR;
    if (worst < 0) {
        fprintf(stderr, "Extraction error, archive corrupted\n");           // csarc.cpp:464-467
        return -1;
    }
    return 0;
}

// What the seven read entry points hand to their one body, dev_read_call.
struct ReadCall {
    CSADevArchive *a;
    const char *const *names;
    int nnames;
    const CSAOptions *opt;
    CSADevFile *files;                         // the files table, of room `cap`
    uint32_t cap;
    bool own_buffers;                          // the entries go to `cap` buffers of the caller's: exactly that many entries, their offsets 0
    const CSADevSlice *layout_slices;          // `sliced` (CSAMI_DeviceReadSlices): per entry, what is read of it
    bool sliced, check_device, stop;           // check_device: refuse without a device first; stop: every task behind its last selected byte
    CSADevReadStats *st;
    CSADevStopStats *stop_stats;
};

// The one read call body below CSAMI_DeviceRead, CSAMI_DeviceReadStop, CSAMI_DeviceReadInto, CSAMI_DeviceCompare, CSAMI_DeviceReadSlices,
// CSAMI_DeviceReadIntoSlices and CSAMI_DeviceCompareSlices: the refusal without a device, the zeroed statistics, the layout, the files
// table, then what only the entry point knows -- prepare(L, B, x, disjoint) fills the caller's side B of the layout L and its own
// statistics x, says whether the buffers are written (`disjoint`: no two selections may meet), and returns 0 or its refusal --, the
// address checks (-1 with nothing launched where CSAMI_CheckSlices refuses the buffers), the waves, and `failed` and the statistics
// copied out.  A refusal leaves every statistics struct zeroed.
template <class X, class Prepare>
int dev_read_call(const ReadCall &c, X *extra, Prepare prepare)
{
    static const CSADevSlice kNone = {0, 0, 0, 0};
    if (c.check_device && CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    CSADevReadStats S;
    CSADevStopStats SS;
    X x;
    memset(&S, 0, sizeof(S));
    memset(&SS, 0, sizeof(SS));
    memset(&x, 0, sizeof(x));
    if (c.st) *c.st = S;
    if (c.stop_stats) *c.stop_stats = SS;
    if (extra) *extra = x;
    DevLayout L;
    const CSADevSlice *ls = !c.sliced ? nullptr : c.layout_slices ? c.layout_slices : &kNone;
    if (!c.a || (c.sliced && c.cap && !c.layout_slices) || !dev_layout(c.a->index, c.a->task_raw, make_selection(c.names, c.nnames), L, ls, ls ? c.cap : 0)
        || (c.own_buffers && L.files.size() != c.cap)) return -1;
    dev_fill_files(L, c.files, c.cap);
    for (uint32_t i = 0; c.own_buffers && c.files && i < c.cap; i++) c.files[i].offset = 0;
    ReadBufs B;
    bool disjoint = true;
    if (const int rc = prepare(L, B, x, disjoint)) return rc;
    if (!dev_bufs_ok(c.a, L, B, disjoint)) return -1;
    std::vector<uint32_t> failed;
    const int rc = dev_read_run(c.a, L, B, c.opt, failed, S, c.stop ? &SS : nullptr);
    for (size_t i = 0; i < failed.size() && i < c.cap; i++) {
        if (B.diffs) B.diffs[i].failed_frags = failed[i];
        if (c.files) c.files[i].failed_frags = failed[i];
    }
    if (c.st) *c.st = S;
    if (c.stop_stats) *c.stop_stats = SS;
    if (extra) *extra = x;
    return rc;
}

// CSAMI_DeviceRead and CSAMI_DeviceReadStop (`stop`, with its stop statistics): the layout's offsets into dst as the entries' pointers
int dev_read(CSADevArchive *a, const char *const *names, int nnames, void *dst, uint64_t dst_cap, const CSAOptions *opt, CSADevFile *files,
             uint32_t cap, CSADevReadStats *st, bool stop, CSADevStopStats *stop_stats)
{
    std::vector<uint8_t *> ptrs;
    std::vector<uint64_t> sizes;
    std::vector<csadev::Slice> bs;
    const ReadCall c = {a, names, nnames, opt, files, cap, false, nullptr, false, stop, stop, st, stop_stats};
    return dev_read_call(c, (CSADevSpreadStats *)nullptr, [&](const DevLayout &L, ReadBufs &B, CSADevSpreadStats &X, bool &) {
        if (dst && dst_cap < L.dst_bytes) return WRITE_ERROR;
        for (const DevFilePlan &f : L.files) {
            ptrs.push_back(dst ? (uint8_t *)dst + f.offset : nullptr);
            sizes.push_back(f.size);
            bs.push_back(whole_slice(f.size));
        }
        if (dst) B.ptrs = ptrs.data();
        B.bslices = bs.data(); B.bsizes = sizes.data(); B.spread = &X;
        return 0;
    });
}

// CSAMI_DeviceReadIntoSlices (diffs == nullptr) and CSAMI_DeviceCompareSlices (compare; diffs may still be NULL, which is refused):
// entry i's side is the slice slices[i] of the buffer ptrs[i] of sizes[i] bytes.
// `whole` (CSAMI_DeviceReadInto, CSAMI_DeviceCompare): `slices` is not looked at -- entry i's side is the first size_i bytes of a buffer
// of sizes[i] (the read), or all sizes[i] bytes of it (the comparison).
int dev_into(CSADevArchive *a, const char *const *names, int nnames, const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices,
             bool whole, uint32_t n, uint32_t flags, const CSAOptions *opt, CSADevFile *files, bool compare, CSADevDiff *diffs, CSADevReadStats *st,
             CSADevStopStats *stop_stats, CSADevSpreadStats *spread_stats)
{
    std::vector<csadev::Slice> bs(n, csadev::Slice{0, 0, 0, 0});
    std::vector<uint64_t> bsz(n, 0), sel(n, 0), lim(n, 0);
    const ReadCall c = {a, names, nnames, opt, files, n, true, nullptr, false, true, (flags & CSAMI_DEV_STOP_EARLY) != 0, st, stop_stats};
    return dev_read_call(c, spread_stats, [&](const DevLayout &L, ReadBufs &B, CSADevSpreadStats &X, bool &disjoint) {
        if (n && ((!whole && (!slices || !sizes)) || (compare && (!diffs || (ptrs && !sizes))))) return -1;
        // the slices, each inside its buffer; the bytes each selects
        for (uint32_t i = 0; i < n; i++) {
            if (!ptrs || !ptrs[i]) continue;
            const uint64_t size = L.files[i].size;
            if (whole) {
                if (!compare && (!sizes || sizes[i] < size)) return WRITE_ERROR;
                bsz[i] = sizes[i];
                sel[i] = compare ? sizes[i] : size;
                bs[i] = whole_slice(sel[i]);
            } else {
                bs[i] = dev_slice(slices[i]);
                bsz[i] = sizes[i];
                if (!csadev::slice_check(bs[i], bsz[i], &sel[i])) return -1;
            }
        }
        for (uint32_t i = 0; i < n; i++) {
            const bool have = ptrs && ptrs[i];
            const uint64_t size = L.files[i].size;
            if (have && !compare && sel[i] < size) return WRITE_ERROR;           // a destination too short for its entry
            lim[i] = std::min(size, sel[i]);
            const uint64_t hull = bs[i].count ? (bs[i].count - 1) * bs[i].stride + bs[i].run : 0;      // (checked by slice_check)
            if (!add_ok(X.selected_bytes, lim[i], &X.selected_bytes)) X.selected_bytes = UINT64_MAX;      // (statistics only: they saturate)
            if (!add_ok(X.hull_bytes, hull, &X.hull_bytes)) X.hull_bytes = UINT64_MAX;
        }
        for (uint32_t i = 0; compare && i < n; i++) {
            const bool have = ptrs && ptrs[i];
            diffs[i].first_diff = UINT64_MAX;
            diffs[i].status = !have ? CSA_DIFF_SKIPPED : sel[i] != L.files[i].size ? CSA_DIFF_SIZE : 0u;
            diffs[i].failed_frags = 0;
        }
        B.ptrs = (uint8_t *const *)ptrs;                                       // (k_frag_compare / k_frag_compare_rows only load from them)
        B.bslices = bs.data(); B.bsizes = bsz.data(); B.spread = &X;
        if (compare) { B.lim = lim.data(); B.diffs = diffs; }
        disjoint = !compare;
        return 0;
    });
}


}   // namespace

extern "C" {

int CSAMI_CheckBuffers(const void *const *ptrs, const uint64_t *sizes, uint32_t n, const void *excl, uint64_t excl_size, int disjoint,
                       uint32_t *bad)
{
    uint32_t worst = UINT32_MAX;
    const uint64_t e0 = (uint64_t)(uintptr_t)excl;
    struct R { uint64_t lo, hi; uint32_t i; };                             // [lo, hi]: hi is the last byte, so a range may end at 2^64
    std::vector<R> rs;
    for (uint32_t i = 0; n && ptrs && sizes && i < n; i++) {
        if (!sizes[i]) continue;
        const uint64_t lo = (uint64_t)(uintptr_t)ptrs[i], hi = lo + (sizes[i] - 1);
        const bool hits = excl_size && lo <= e0 + (excl_size - 1) && e0 <= hi;    // (an excl that itself wraps is the caller's to refuse)
        if (!lo || hi < lo || hits) { worst = std::min(worst, i); continue; }
        if (disjoint) rs.push_back(R{lo, hi, i});
    }
    if (n && (!ptrs || !sizes)) worst = 0;
    // ranges in address order: one that begins at or before the furthest end so far overlaps the range that reaches it.  Every
    // range that overlaps another is found as one of the two: the range next behind it begins inside it, or inside a longer one.
    std::sort(rs.begin(), rs.end(), [](const R &a, const R &b) { return a.lo != b.lo ? a.lo < b.lo : a.i < b.i; });
    for (size_t k = 1, far = 0; k < rs.size(); k++) {
        if (rs[k].lo <= rs[far].hi) worst = std::min(worst, std::min(rs[k].i, rs[far].i));
        if (rs[k].hi > rs[far].hi) far = k;
    }
    if (worst == UINT32_MAX) return 0;
    if (bad) *bad = worst;
    return -1;
}

int CSAMI_DeviceRead(CSADevArchive *a, const char *const *names, int nnames, void *dst, uint64_t dst_cap,
                     const CSAOptions *opt, CSADevFile *files, uint32_t cap, CSADevReadStats *st)
{
    return dev_read(a, names, nnames, dst, dst_cap, opt, files, cap, st, false, nullptr);
}

int CSAMI_DeviceReadStop(CSADevArchive *a, const char *const *names, int nnames, void *dst, uint64_t dst_cap,
                         const CSAOptions *opt, CSADevFile *files, uint32_t cap, CSADevReadStats *st, CSADevStopStats *stop_stats)
{
    return dev_read(a, names, nnames, dst, dst_cap, opt, files, cap, st, true, stop_stats);
}

int CSAMI_CheckSlices(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, uint32_t n, const void *excl, uint64_t excl_size,
                      int disjoint, uint32_t *bad)
{
    uint32_t worst = UINT32_MAX;
    const uint64_t e0 = (uint64_t)(uintptr_t)excl;
    struct H { uint64_t lo, hi, run, stride; uint32_t i; bool rows; };     // the hull [lo, hi]: hi is its last byte; rows: count > 1
    std::vector<H> hs;
    for (uint32_t i = 0; n && ptrs && sizes && slices && i < n; i++) {
        csadev::Slice s = dev_slice(slices[i]);
        uint64_t bytes, lo;
        if (!csadev::slice_check(s, sizes[i], &bytes)) { worst = std::min(worst, i); continue; }
        if (!s.count) continue;
        const uint64_t hull = (s.count - 1) * s.stride + s.run;           // (checked by slice_check)
        if (!ptrs[i] || !add_ok((uint64_t)(uintptr_t)ptrs[i], s.offset, &lo)) { worst = std::min(worst, i); continue; }
        const uint64_t hi = lo + (hull - 1);
        const bool hits = excl_size && lo <= e0 + (excl_size - 1) && e0 <= hi;
        if (hi < lo || hits) { worst = std::min(worst, i); continue; }
        if (disjoint) hs.push_back(H{lo, hi, s.run, s.stride, i, s.count > 1});
    }
    if (n && (!ptrs || !sizes || !slices)) worst = 0;
    // Two hulls that overlap are apart only where their selected bytes provably do not meet: under one stride S (a slice of one run
    // takes the other's) A selects addresses of residues [a, a + run_A) and B of [a + d, a + d + run_B) modulo S, so d >= run_A and
    // d + run_B <= S keeps them apart -- column blocks of one matrix, a byte range inside one gap.  No walk over the rows.
    auto apart = [](const H &A, const H &B) {
        if ((!A.rows && !B.rows) || (A.rows && B.rows && A.stride != B.stride)) return false;
        const uint64_t S = A.rows ? A.stride : B.stride;
        const uint64_t d = (B.lo - A.lo) % S;                              // (the sweep hands the hull with the lower start in as A)
        return d >= A.run && B.run <= S && d <= S - B.run;
    };
    // hulls in address order; `open` holds those that reach the one at hand, each of which overlaps it: a hull is dropped from it
    // once, and otherwise costs one look per overlapping pair
    std::sort(hs.begin(), hs.end(), [](const H &a, const H &b) { return a.lo != b.lo ? a.lo < b.lo : a.i < b.i; });
    std::vector<size_t> open;
    for (size_t k = 0; k < hs.size(); k++) {
        size_t w = 0;
        for (size_t j : open) {
            if (hs[j].hi < hs[k].lo) continue;
            open[w++] = j;
            if (!apart(hs[j], hs[k])) worst = std::min(worst, std::min(hs[j].i, hs[k].i));
        }
        open.resize(w);
        open.push_back(k);
    }
    if (worst == UINT32_MAX) return 0;
    if (bad) *bad = worst;
    return -1;
}

int CSAMI_DeviceReadIntoSlices(CSADevArchive *a, const char *const *names, int nnames, void *const *ptrs, const uint64_t *sizes,
                               const CSADevSlice *slices, uint32_t n, uint32_t flags, const CSAOptions *opt, CSADevFile *files,
                               CSADevReadStats *st, CSADevStopStats *stop_stats, CSADevSpreadStats *spread_stats)
{
    return dev_into(a, names, nnames, (const void *const *)ptrs, sizes, slices, false, n, flags, opt, files, false, nullptr, st, stop_stats, spread_stats);
}

int CSAMI_DeviceCompareSlices(CSADevArchive *a, const char *const *names, int nnames, const void *const *ptrs, const uint64_t *sizes,
                              const CSADevSlice *slices, uint32_t n, uint32_t flags, const CSAOptions *opt, CSADevFile *files,
                              CSADevDiff *diffs, CSADevReadStats *st, CSADevStopStats *stop_stats, CSADevSpreadStats *spread_stats)
{
    return dev_into(a, names, nnames, ptrs, sizes, slices, false, n, flags, opt, files, true, diffs, st, stop_stats, spread_stats);
}

// the two calls above with whole-buffer slices
int CSAMI_DeviceReadInto(CSADevArchive *a, const char *const *names, int nnames, void *const *ptrs, const uint64_t *caps, uint32_t n,
                         uint32_t flags, const CSAOptions *opt, CSADevFile *files, CSADevReadStats *st, CSADevStopStats *stop_stats)
{
    return dev_into(a, names, nnames, (const void *const *)ptrs, caps, nullptr, true, n, flags, opt, files, false, nullptr, st, stop_stats, nullptr);
}

int CSAMI_DeviceCompare(CSADevArchive *a, const char *const *names, int nnames, const void *const *ptrs, const uint64_t *sizes, uint32_t n,
                        uint32_t flags, const CSAOptions *opt, CSADevFile *files, CSADevDiff *diffs, CSADevReadStats *st,
                        CSADevStopStats *stop_stats)
{
    return dev_into(a, names, nnames, ptrs, sizes, nullptr, true, n, flags, opt, files, true, diffs, st, stop_stats, nullptr);
}

int CSAMI_DeviceReadSlices(CSADevArchive *a, const char *const *names, int nnames, const CSADevSlice *slices, void *const *ptrs,
                           const uint64_t *caps, uint32_t n, uint32_t flags, const CSAOptions *opt, CSADevFile *files, CSADevReadStats *st,
                           CSADevStopStats *stop_stats, CSADevSliceStats *slice_stats)
{
    const ReadCall c = {a, names, nnames, opt, files, n, true, slices, true, true, (flags & CSAMI_DEV_STOP_EARLY) != 0, st, stop_stats};
    std::vector<csadev::Slice> bs;
    return dev_read_call(c, slice_stats, [&](const DevLayout &L, ReadBufs &B, CSADevSliceStats &SL, bool &) {
        SL.touched_bytes = L.touched_bytes;
        for (uint32_t i = 0; i < n; i++) {
            if (ptrs && ptrs[i] && (!caps || caps[i] < L.slice_bytes[i])) return WRITE_ERROR;
            if (!add_ok(SL.selected_bytes, L.slice_bytes[i], &SL.selected_bytes)) return -1;
            bs.push_back(whole_slice(L.slice_bytes[i]));
        }
        B.ptrs = (uint8_t *const *)ptrs;
        B.bslices = bs.data(); B.bsizes = L.slice_bytes.data();
        B.slice_stats = &SL;
        return 0;
    });
}

int CSAMI_DeviceReadDigests(CSADevArchive *a, const CSAOptions *opt, CSADevDigest *digests_out, uint64_t digests_cap, const CSADevDigest *expect,
                            CSADevReadStats *st, CSADevDigestStats *ds)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    DigestCall dg = {digests_out, expect, CSADevDigestStats()};
    memset(&dg.ds, 0, sizeof(dg.ds));
    g_digest_ms[0] = g_digest_ms[1] = 0;
    if (ds) *ds = dg.ds;
    std::vector<uint64_t> sizes;
    std::vector<csadev::Slice> bs;
    const ReadCall c = {a, nullptr, 0, opt, nullptr, 0, false, nullptr, false, false, false, st, nullptr};
    const int rc = dev_read_call(c, (CSADevSpreadStats *)nullptr, [&](const DevLayout &L, ReadBufs &B, CSADevSpreadStats &X, bool &) {
        const uint64_t bytes = L.index_frags * sizeof(CSADevDigest);
        if ((!digests_out && !expect) || ranges_meet(digests_out, bytes, a->arc, a->arc_size) || ranges_meet(expect, bytes, a->arc, a->arc_size)
            || ranges_meet(digests_out, bytes, expect, bytes)) return -1;
        if (digests_out && digests_cap < L.index_frags) return WRITE_ERROR;
        for (const DevFilePlan &f : L.files) {
            sizes.push_back(f.size);
            bs.push_back(whole_slice(f.size));
        }
        B.bslices = bs.data(); B.bsizes = sizes.data(); B.spread = &X;
        B.dg = &dg;
        dg.ds.first_mismatch = UINT64_MAX;
        return 0;
    });
    if (ds) *ds = dg.ds;
    return rc;
}

void CSAMI_DeviceDigestKernelMs(double ms[2])
{
    ms[0] = g_digest_ms[0]; ms[1] = g_digest_ms[1];
}

void CSAMI_DeviceKernelMs(const CSADevArchive *a, double ms[3])
{
    for (int i = 0; i < 3; i++) ms[i] = a ? a->kernel_ms[i] : 0;
}

void CSAMI_DeviceClose(CSADevArchive *a) { delete a; }

}   // extern "C"

namespace {

// the strict host-only plan of CSAMI_PlanDeviceLayout / CSAMI_PlanDeviceStops: false for an index that does not parse, whose sizes
// wrap, or with an archive block outside [0, arc_size).  L.files point into `index`.
bool dev_plan_strict(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                     Index &index, DevLayout &L, const CSADevSlice *slices = nullptr, size_t nslices = 0)
{
    BlockIndex abindex;
    std::map<uint64_t, uint64_t> raw;
    if (!raw_index || !unpack_index(index, abindex, raw_index, raw_size) || !dev_task_sizes(index, raw)) return false;
    for (const auto &kv : abindex)
        for (const Extent &x : kv.second) {
            uint64_t end;
            if (!add_ok(x.off, x.size, &end) || end > arc_size) return false;
        }
    return dev_layout(index, raw, make_selection(names, nnames), L, slices, nslices);
}

// what CSAMI_PlanDeviceStops and CSAMI_PlanDeviceSlices hand out of a layout; -1 for a task whose stop cannot be
int dev_fill_stops(const DevLayout &L, uint64_t *bids, uint64_t *stops, uint64_t *raws, uint32_t cap, uint32_t *n_tasks)
{
    for (const DevTask &t : L.tasks)
        if (t.stop == 0 || t.stop > t.raw) return -1;                       // (a selected fragment past its task: cannot be, by construction)
    for (size_t i = 0; i < L.tasks.size() && i < cap; i++) {
        if (bids) bids[i] = L.tasks[i].bid;
        if (stops) stops[i] = L.tasks[i].stop;
        if (raws) raws[i] = L.tasks[i].raw;
    }
    if (n_tasks) *n_tasks = (uint32_t)L.tasks.size();
    return 0;
}

}   // namespace

extern "C" {

int CSAMI_PlanDeviceLayout(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                           CSADevFile *files, uint32_t cap, uint32_t *n_files, uint64_t *dst_bytes,
                           uint64_t *task_raw_sizes, uint32_t task_cap, uint32_t *n_tasks)
{
    Index index;
    DevLayout L;
    if (!dev_plan_strict(raw_index, raw_size, arc_size, names, nnames, index, L)) return -1;
    dev_fill_files(L, files, cap);
    // the names: inside raw_index, where the parse above found them (the first entry of a name wins, as in the map)
    std::map<std::string, const char *> where;
    uint64_t pos = 4;
    for (uint32_t i = 0, n = (uint32_t)load_le(raw_index, 4); i < n; i++) {
        const uint32_t ln = (uint32_t)load_le(raw_index + pos, 4);
        const char *p = (const char *)raw_index + pos + 4;
        where.insert(std::make_pair(std::string(p, ln), p));
        const int nfr = (int8_t)raw_index[pos + 4 + ln + 24];
        pos += 4 + (uint64_t)ln + 25 + 32ull * (uint64_t)nfr;
    }
    for (size_t i = 0; files && i < L.files.size() && i < cap; i++) files[i].name = where[L.files[i].it->first];
    if (n_files) *n_files = (uint32_t)L.files.size();
    if (dst_bytes) *dst_bytes = L.dst_bytes;
    for (size_t i = 0; task_raw_sizes && i < L.tasks.size() && i < task_cap; i++) task_raw_sizes[i] = L.tasks[i].raw;
    if (n_tasks) *n_tasks = (uint32_t)L.tasks.size();
    return 0;
}

int CSAMI_PlanDeviceStops(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                          uint64_t *bids, uint64_t *stops, uint64_t *raws, uint32_t cap, uint32_t *n_tasks)
{
    Index index;
    DevLayout L;
    if (!dev_plan_strict(raw_index, raw_size, arc_size, names, nnames, index, L)) return -1;
    return dev_fill_stops(L, bids, stops, raws, cap, n_tasks);
}

int CSAMI_PlanDeviceSlices(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const char *const *names, int nnames,
                           const CSADevSlice *slices, uint32_t n, uint64_t *bids, uint64_t *stops, uint64_t *raws, uint32_t cap,
                           uint32_t *n_tasks, uint32_t *n_touched)
{
    static const CSADevSlice kNone = {0, 0, 0, 0};
    Index index;
    DevLayout L;
    if ((n && !slices) || !dev_plan_strict(raw_index, raw_size, arc_size, names, nnames, index, L, slices ? slices : &kNone, n)) return -1;
    if (n_touched) *n_touched = (uint32_t)L.touched_frags;
    return dev_fill_stops(L, bids, stops, raws, cap, n_tasks);
}

}   // extern "C"

// ---------------------------------------------------------------------------------------------
// device-resident write: CSAMI_DeviceWritePlan / CSAMI_DeviceWrite (include/csa_mi355x.h).
// Host side: the index from the caller's table, the plan CSA_Add makes (plan_index), the validation of every size, the piece
// tables, arc_end, the index and the header.  The bytes move in csa_dev_kernels.hip (k_frag_pieces, k_frag_fold, k_block_table,
// k_gather_extents; tables and walks: csa_dev_read.h, csa_dev_write.h) and in CSCMI_EncodeDeviceBatch.  All of them are one path
// over a device pointer and a slice per entry (CSAMI_DeviceWriteSlices): CSAMI_DeviceWrite and CSAMI_DeviceWriteFrom hand in whole
// entries; where a slice has rows, a task's fragments are gathered across the run borders by k_frag_rows.
// CSAMI_DeviceUpdateDigests is that path with the fragment digests (csa_dev_digest.h): one DigestPass over the plan's fragments before the
// waves, for the table the call hands out and for the comparison with the base's table under CSAMI_UPDATE_TRUST_DIGESTS.
// CSAMI_DeviceUpdate is that path with a base archive: the tasks of the plan that are tasks of the base (update_candidates) and whose
// bytes are still the base's (dev_check_wave) are placed from the base instead of encoded; CSAMI_DeviceWriteSlices is it without one.
// CSAMI_DeviceUpdateInPlace is the update whose new archive takes the base's place in the caller's buffer: the same body (dev_update)
// with the steps in the order that puts every refusal before the first store, and the reused streams moved by k_move_extents.
// ---------------------------------------------------------------------------------------------
namespace {

thread_local double g_write_ms[4] = {0, 0, 0, 0};      // CSAMI_DeviceWriteKernelMs

// The caller's table as an index, and its plan.  -1 for a table the host refuses; where the entries' bytes lie is not looked at.
int plan_write(AddPlan &P, const CSADevFile *files, uint32_t n_files, const CSAOptions *opt, uint64_t *raw_bytes)
{
    if (opt) P.o = *opt; else CSA_OptionsInit(&P.o);
    if (n_files && !files) return -1;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n_files; i++) {
        const CSADevFile &f = files[i];
        if (!f.name || f.esize < 0) return -1;
        const std::string name(f.name);
        if (!name.empty() && name[name.size() - 1] == '/' && f.esize != 0) return -1;
        if (!add_ok(sum, (uint64_t)f.esize, &sum) || sum > (1ull << 60)) return -1;   // (every later sum of sizes stays far from 2^64)
        auto ins = P.index.insert(std::make_pair(name, Entry()));
        if (!ins.second) return -1;
        Entry &e = ins.first->second;
        e.edate = f.edate; e.esize = f.esize; e.eattr = f.eattr; e.row = i;
    }
    const int rc = plan_index(P);
    if (raw_bytes) { *raw_bytes = 0; for (const Task &t : P.tasks) *raw_bytes += t.total; }
    return rc;
}

// CSAMI_DeviceUpdate: what the call knows of a task of the new plan
struct UpdTask {
    uint64_t base_bid = UINT64_MAX;
    uint32_t status = CSA_UPD_NEW;
    bool candidate = false;                    // the host step found its base task, and no later step has ruled it out yet
    bool have_sums = false;                    // its fragments' checksums are the caller's bytes' (the check under TRUST_SUMS summed them)
    std::vector<uint32_t> base_sums;           // candidate: the base index's checksum of each of its fragments, in the task's order
    std::vector<uint64_t> base_pos;            //            and each one's place in the base index (= in the base's digest table)
    bool digest_changed = false;               // CSAMI_UPDATE_TRUST_DIGESTS: a fragment's digest is not the base table's
    std::vector<Extent> ext;                   // candidate: the base stream's archive blocks, clipped to the base buffer
    uint64_t stream = 0;                       //            and their bytes, the 10 property bytes included
};
struct UpdateCtx {
    CSADevArchive *base = nullptr;
    bool trust = false;                        // nothing is decoded: CSAMI_UPDATE_TRUST_SUMS, CSAMI_UPDATE_TRUST_DIGESTS
    bool digests = false;                      // CSAMI_UPDATE_TRUST_DIGESTS: the digest pass decides, the base's checksums decide nothing
    std::vector<UpdTask> tasks;
    CSADevUpdateStats U;
    double ms = 0;                             // HIP-event time of the check waves' launches
    bool reused(size_t task) const { return tasks[task].status == CSA_UPD_REUSED; }
};

// The candidates of CSAMI_DeviceUpdate / CSAMI_PlanDeviceUpdate (host): task i of the plan is a candidate for base task bids[i] when
// it holds a byte and the set of its fragments (name, offset in the entry, size, posblock) is the set of ALL fragments of the base
// index with that bid; UINT64_MAX where there is none.  One map from (name, offset) to the base's fragments there, one look per
// fragment of the plan: no task is compared with another.  Sets posblock of every fragment of the plan (csa_io.h:239); sums[i]
// gets the base's checksums of a candidate's fragments, in the task's order, and pos[i] (pos != NULL) their places in the base index.
// Returns the number of candidates.
uint32_t update_candidates(const Index &base, AddPlan &P, std::vector<uint64_t> &bids, std::vector<std::vector<uint32_t>> &sums,
                           std::vector<std::vector<uint64_t>> *pos = nullptr)
{
    struct BaseFrag { uint64_t bid, size, posblock; uint32_t checksum; uint64_t idx; };
    uint64_t idx = 0;
    std::map<std::pair<std::string, uint64_t>, std::vector<BaseFrag>> where;
    std::map<uint64_t, uint64_t> nfrags;
    for (const auto &kv : base)
        for (const CSAFrag &f : kv.second.frags) {
            where[std::make_pair(kv.first, (uint64_t)f.posfile)].push_back(BaseFrag{f.bid, f.size, f.posblock, f.checksum, idx++});
            nfrags[f.bid]++;
        }
    bids.assign(P.tasks.size(), UINT64_MAX);
    sums.assign(P.tasks.size(), std::vector<uint32_t>());
    if (pos) pos->assign(P.tasks.size(), std::vector<uint64_t>());
    uint32_t n = 0;
    for (size_t ti = 0; ti < P.tasks.size(); ti++) {
        Task &t = P.tasks[ti];
        uint64_t cum = 0;
        for (FilePiece &f : t.files) { f.posblock = cum; cum += f.size; }
        if (!t.total) continue;
        uint64_t bid = UINT64_MAX;
        std::vector<uint32_t> cs;
        std::vector<uint64_t> at;
        for (const FilePiece &f : t.files) {
            const BaseFrag *hit = nullptr;
            auto w = where.find(std::make_pair(f.it->first, f.off));
            if (w != where.end())
                for (const BaseFrag &b : w->second)
                    if (b.size == f.size && b.posblock == f.posblock && (bid == UINT64_MAX || b.bid == bid)) { hit = &b; break; }
            if (!hit) break;
            bid = hit->bid;
            cs.push_back(hit->checksum);
            at.push_back(hit->idx);
        }
        if (cs.size() != t.files.size() || nfrags[bid] != t.files.size()) continue;
        bids[ti] = bid;
        sums[ti].swap(cs);
        if (pos) (*pos)[ti].swap(at);
        n++;
    }
    return n;
}

struct WriteCtx {
    UpdateCtx *upd = nullptr;                  // CSAMI_DeviceUpdate with a base: the tasks whose streams are copied, not encoded
    const void *const *ptrs = nullptr;        // entry `row` of the caller's table: the bytes that slices[row], checked, selects of
    const csadev::Slice *slices = nullptr;     // the buffer at ptrs[row], packed row after row
    uint8_t *arc = nullptr;
    uint64_t arc_cap = 0, arc_end = kHeaderSize;
    const uint8_t *buf(const FilePiece &f) const { return (const uint8_t *)ptrs[f.it->second.row]; }
    const csadev::Slice &slice(const FilePiece &f) const { return slices[f.it->second.row]; }
    int64_t slack = -1;                        // CSA_DEVWRITE_SLACK, -1: not set
    CSADevWriteStats S;
    CSADevGatherStats G;
    DevTimer tm;
    BlockIndex abindex;
};

uint64_t stream_cap(const WriteCtx &W, uint64_t raw)
{
    return W.slack >= 0 ? raw / 4 + (uint64_t)W.slack : raw + raw / 8 + 65536;
}

bool dev_upload(WriteCtx &W, DevBuf &b, const void *p, uint64_t n)
{
    W.S.upload_bytes += n;
    return b.upload(p, n);
}

// CSCMI_EncodeDeviceBatch over jobs whose dst is scratch of this layer; a job whose scratch was too small once more, alone, into a
// larger one (kept in `more` until its stream is placed)
int dev_encode(WriteCtx &W, std::vector<CSCMIDevEncode> &jobs, std::list<DevBuf> &more)
{
    const double t0 = now_s();
    CSCMIDevEncodeStats es;
    memset(&es, 0, sizeof(es));
    int rc = CSCMI_EncodeDeviceBatch((int)jobs.size(), jobs.data(), &es) == 0 ? 0 : CSCMI_DEVICE_ERROR;
    W.S.encode_launches += es.launches; W.S.readback_bytes += es.readback_bytes;
    for (size_t i = 0; rc == 0 && i < jobs.size(); i++) {
        CSCMIDevEncode &j = jobs[i];
        if (j.rc == WRITE_ERROR) {
            more.emplace_back();
            const uint64_t cap = 2 * (uint64_t)j.src_size + (1u << 20);
            if (!more.back().alloc(cap)) { rc = CSCMI_DEVICE_ERROR; break; }
            j.dst = more.back().p; j.dst_cap = (size_t)cap; j.produced = 0; j.rc = 0;
            W.S.retries++;
            memset(&es, 0, sizeof(es));
            if (CSCMI_EncodeDeviceBatch(1, &j, &es) != 0) rc = CSCMI_DEVICE_ERROR;
            W.S.encode_launches += es.launches; W.S.readback_bytes += es.readback_bytes;
        }
        if (j.rc != 0) rc = CSCMI_DEVICE_ERROR;
    }
    W.S.seconds_encode += now_s() - t0;
    return rc;
}

// One stream to place: an encoded one (job: its property bytes come from the host, its stream lies in scratch), or one of the base
// archive of CSAMI_DeviceUpdate (ext: its archive blocks in `base`, the 10 property bytes in front of the first; stream: their bytes)
struct Placed {
    const CSCMIDevEncode *job;
    const std::vector<Extent> *ext;
    const uint8_t *base;
    uint64_t stream;
    uint64_t bytes() const { return job ? CSC_PROP_SIZE + (uint64_t)job->produced : stream; }
};

// Every stream of `items` to arc + arc_end, in order, with one launch; `hdr` (NULL, or the 24 header bytes) goes to arc + 0 with it.
// at[k]: where stream k begins.  WRITE_ERROR, with nothing launched, if it would pass arc_cap.
int dev_place(WriteCtx &W, const std::vector<Placed> &items, const uint8_t *hdr, std::vector<uint64_t> *at = nullptr)
{
    using namespace csadev;
    const uint64_t lead = hdr ? kHeaderSize : 0;
    uint64_t end = W.arc_end;
    for (const Placed &it : items)
        if (!add_ok(end, it.bytes(), &end)) return WRITE_ERROR;
    if (end > W.arc_cap) return WRITE_ERROR;
    // the bytes that come from the host: [the header] and the property bytes of every encoded stream
    std::vector<uint8_t> host(hdr, hdr + lead);
    for (const Placed &it : items) {
        if (!it.job) continue;
        uint8_t props[CSC_PROP_SIZE];
        CSCEnc_WriteProperties(&it.job->props, props, 0);                    // csa_worker.cpp:38-42
        host.insert(host.end(), props, props + CSC_PROP_SIZE);
    }
    DevBuf d_host, d_gp;
    if (!dev_upload(W, d_host, host.data(), host.size())) return CSCMI_DEVICE_ERROR;
    std::vector<CopyPiece> gp;
    if (hdr) gp.push_back(CopyPiece{(const uint8_t *)d_host.p, W.arc, (uint32_t)kHeaderSize, 0});
    uint64_t pos = W.arc_end, hp = lead;
    auto put = [&](uint64_t, const CopyPiece &p) { gp.push_back(p); };
    if (at) at->clear();
    for (const Placed &it : items) {
        if (at) at->push_back(pos);
        if (it.job) {
            gp.push_back(CopyPiece{(const uint8_t *)d_host.p + hp, W.arc + pos, CSC_PROP_SIZE, 0});
            piece_split((const uint8_t *)it.job->dst, W.arc + pos + CSC_PROP_SIZE, it.job->produced, kGatherPiece, put);
            hp += CSC_PROP_SIZE;
            pos += it.bytes();
        } else {
            for (const Extent &x : *it.ext) { piece_split(it.base + x.off, W.arc + pos, x.size, kGatherPiece, put); pos += x.size; }
        }
    }
    if (gp.size() > 0x7FFFFFFFull || !dev_upload(W, d_gp, gp.data(), gp.size() * sizeof(CopyPiece))) return CSCMI_DEVICE_ERROR;
    if (!W.tm.timed(&g_write_ms[3], W.S.launches, [&] { launch_gather_extents(d_gp.p, (uint32_t)gp.size(), W.tm.st); })) return CSCMI_DEVICE_ERROR;
    W.arc_end = pos;
    return 0;
}

// The front half of a wave, tasks [first, first + count) of the plan, which the write and the update in place share: where each
// task's raw bytes lie, the gather and the sums, the encode into scratch of this layer.  jobs[job_of[k]] is task first + k's (a
// reused task has none); the scratch lives as long as this object.
struct WaveStreams {
    DevBuf d_gat, d_scr;
    std::list<DevBuf> more;
    std::vector<CSCMIDevEncode> jobs;
    std::vector<size_t> job_of;
    int encode(WriteCtx &W, AddPlan &P, size_t first, size_t count);       // 0 or CSCMI_DEVICE_ERROR
};

int WaveStreams::encode(WriteCtx &W, AddPlan &P, size_t first, size_t count)
{
    using namespace csadev;
    auto reused = [&](size_t k) { return W.upd && W.upd->reused(first + k); };
    // 1. where each task's raw bytes lie: one range of one entry that lies inside one run of its slice is encoded where it is,
    // anything else is gathered
    std::vector<const uint8_t *> in(count, nullptr);
    std::vector<uint64_t> gat_off(count, 0);
    std::vector<uint8_t> gathered(count, 0);
    uint64_t gat_bytes = 0, npieces = 0;
    for (size_t k = 0; k < count; k++) {
        Task &t = P.tasks[first + k];
        uint64_t cum = 0;
        size_t nonempty = 0;
        bool in_run = false;
        for (FilePiece &f : t.files) {
            f.posblock = cum;                                                // csa_io.h:239
            cum += f.size;
            if (reused(k)) continue;
            if (f.size) {
                uint64_t src;
                nonempty++;
                in_run = gather_whole(W.slice(f), f.off, f.size, &src);
                in[k] = W.buf(f) + src;
            }
            npieces += piece_count(f.size, kFragPiece);
        }
        if (nonempty > 1 || (nonempty == 1 && !in_run)) {
            gathered[k] = 1;
            gat_off[k] = gat_bytes;
            gat_bytes += (t.total + 255) & ~255ull;
            W.G.gathered_tasks++;
        } else if (nonempty) {
            W.G.inplace_tasks++;
        }
    }
    if (npieces > 0x7FFFFFFFull) return CSCMI_DEVICE_ERROR;
    if (gat_bytes && !d_gat.alloc(gat_bytes)) return CSCMI_DEVICE_ERROR;

    // 2. gather and sum in one pass: the fragments of the gathered tasks, whose pieces are stored, first -- through k_frag_rows if
    // one of them crosses a run border, else as the CopyPieces they all are; then, in a launch of their own, those of the tasks
    // encoded where they lie, whose pieces are only summed (but for a task whose fragments the update's check has summed already)
    {
        FragTables T(FragTables::kGathered);
        std::vector<FilePiece *> ff_piece;
        for (size_t k = 0; k < count; k++) {
            if (!gathered[k]) continue;
            for (FilePiece &f : P.tasks[first + k].files) {
                f.checksum = 0;
                if (!f.size) continue;                                           // adler32 of nothing, seed 0
                if (!T.add_gathered(W.buf(f), (uint8_t *)d_gat.p + gat_off[k] + f.posblock, W.slice(f), f.off, f.size, W.G)) return CSCMI_DEVICE_ERROR;
                ff_piece.push_back(&f);
            }
            in[k] = (const uint8_t *)d_gat.p + gat_off[k];
        }
        for (size_t k = 0; k < count; k++) {
            if (gathered[k] || reused(k) || (W.upd && W.upd->tasks[first + k].have_sums)) continue;
            for (FilePiece &f : P.tasks[first + k].files) {
                f.checksum = 0;
                if (!f.size) continue;
                if (!T.add_summed(in[k], f.size)) return CSCMI_DEVICE_ERROR;
                ff_piece.push_back(&f);
            }
        }
        if (!T.frags.empty()) {
            W.G.plain_pieces += T.summed();
            std::vector<FragResult> res;
            if (!T.sum(LaunchSlot{W.tm, &g_write_ms[0], &g_write_ms[1], W.S.launches}, false, &W.S.upload_bytes, res)) return CSCMI_DEVICE_ERROR;
            W.S.readback_bytes += res.size() * sizeof(FragResult);
            for (size_t i = 0; i < res.size(); i++) ff_piece[i]->checksum = res[i].adler;        // csa_io.h:250
        }
    }

    // 3. encode: csa_worker.cpp:23-56 for every task of the wave that is not reused at once, into scratch of this layer
    jobs.clear();
    job_of.assign(count, SIZE_MAX);
    uint64_t scr_bytes = 0;
    std::vector<uint64_t> scr_off(count, 0);
    for (size_t k = 0; k < count; k++) {
        if (reused(k)) continue;
        scr_off[k] = scr_bytes;
        scr_bytes += (stream_cap(W, P.tasks[first + k].total) + 255) & ~255ull;
    }
    if (!d_scr.alloc(scr_bytes)) return CSCMI_DEVICE_ERROR;
    for (size_t k = 0; k < count; k++) {
        if (reused(k)) continue;
        const Task &t = P.tasks[first + k];
        CSCMIDevEncode j;
        memset(&j, 0, sizeof(j));
        CSCEncProps_Init(&j.props, (uint32_t)std::min<uint64_t>(P.o.dict_size, t.total), P.o.level);   // csa_worker.cpp:35
        j.src = t.total ? (const void *)in[k] : d_scr.p;                     // (no byte of it is loaded when the task is empty)
        j.src_size = (size_t)t.total;
        j.dst = (uint8_t *)d_scr.p + scr_off[k];
        j.dst_cap = (size_t)stream_cap(W, t.total);
        job_of[k] = jobs.size();
        jobs.push_back(j);
    }
    return jobs.empty() ? 0 : dev_encode(W, jobs, more);
}

// One k_block_table launch over `bj` (job i is task task[i] of the plan, a reused one where reused[i]) and what the host reads
// back of it: br[i], and the block sizes of all jobs back to back in `sizes`.  0, CSCMI_DEVICE_ERROR, or -1: a reused stream does
// not end at its length.
int dev_block_tables(WriteCtx &W, const std::vector<csadev::BlockTableJob> &bj, const std::vector<size_t> &task, const std::vector<uint8_t> &reused,
                     std::vector<csadev::BlockTableRes> &br, std::vector<uint64_t> &sizes)
{
    using namespace csadev;
    const size_t count = bj.size();
    uint64_t slots = 0;
    for (const BlockTableJob &j : bj) slots += j.max_blocks;
    br.assign(count, BlockTableRes{0, 0});
    DevBuf d_bj, d_slots, d_res, d_sizes;
    if (!dev_upload(W, d_bj, bj.data(), bj.size() * sizeof(BlockTableJob)) || !d_slots.alloc(slots * 8) || !d_res.alloc(count * sizeof(BlockTableRes))
        || !d_sizes.alloc(slots * 8)) return CSCMI_DEVICE_ERROR;
    if (!W.tm.timed(&g_write_ms[2], W.S.launches, [&] { launch_block_table(d_bj.p, (uint32_t)count, d_slots.p, d_res.p, d_sizes.p, W.tm.st); }))
        return CSCMI_DEVICE_ERROR;
    if (!HIP_OK(hipMemcpy(br.data(), d_res.p, count * sizeof(BlockTableRes), hipMemcpyDeviceToHost))) return CSCMI_DEVICE_ERROR;
    W.S.readback_bytes += count * sizeof(BlockTableRes);
    uint64_t nb = 0;
    for (size_t k = 0; k < count; k++) {
        if (br[k].status != kTableOk || br[k].nblocks > bj[k].max_blocks) {
            if (reused[k]) {
                fprintf(stderr, "csa-mi355x: task %zu: the stream reused from the base archive does not end at its length (block table status %u)\n",
                        task[k], br[k].status);
                return -1;
            }
            fprintf(stderr, "csa-mi355x: task %zu: its stream does not end where its encoder said (block table status %u)\n", task[k], br[k].status);
            return CSCMI_DEVICE_ERROR;
        }
        nb += br[k].nblocks;
    }
    sizes.resize(nb);
    if (nb && !HIP_OK(hipMemcpy(sizes.data(), d_sizes.p, nb * 8, hipMemcpyDeviceToHost))) return CSCMI_DEVICE_ERROR;
    W.S.readback_bytes += nb * 8;
    W.S.blocks += nb;
    return 0;
}

// One wave: tasks [first, first + count) of the plan.  0, WRITE_ERROR, CSCMI_DEVICE_ERROR, or -1 (CSAMI_DeviceUpdate: a reused
// stream does not end at its length).  A task CSAMI_DeviceUpdate reuses is neither gathered nor summed nor encoded: its stream is
// placed from the base archive beside the encoded ones, and its block table taken where it was placed.
int dev_write_wave(WriteCtx &W, AddPlan &P, size_t first, size_t count)
{
    using namespace csadev;
    auto reused = [&](size_t k) { return W.upd && W.upd->reused(first + k); };
    // 1. - 3. gather, sum, encode
    WaveStreams E;
    int rc = E.encode(W, P, first, count);
    if (rc) return rc;
    const std::vector<CSCMIDevEncode> &jobs = E.jobs;
    const std::vector<size_t> &job_of = E.job_of;

    // 4. placement (csa_io.h:559-573; id == task index, csarc.cpp:393-394): it needs the streams' sizes alone
    std::vector<Placed> items(count);
    std::vector<uint64_t> at;
    for (size_t k = 0; k < count; k++) {
        if (reused(k)) { const UpdTask &u = W.upd->tasks[first + k]; items[k] = Placed{nullptr, &u.ext, W.upd->base->arc, u.stream}; }
        else items[k] = Placed{&jobs[job_of[k]], nullptr, nullptr, 0};
    }
    rc = dev_place(W, items, nullptr, &at);
    if (rc) return rc;

    // 5. block tables: BlockSink::put over the Write sizes the file path would have seen -- of an encoded stream where it lies in
    // scratch, of a reused one where it was placed, so that its table is this writer's whatever cut the base into blocks
    std::vector<BlockTableJob> bj(count);
    uint64_t slots = 0;
    for (size_t k = 0; k < count; k++) {
        CSCProps props;
        if (reused(k)) CSCEncProps_Init(&props, (uint32_t)std::min<uint64_t>(P.o.dict_size, P.tasks[first + k].total), P.o.level);   // (its 10 bytes are these props')
        else props = jobs[job_of[k]].props;
        const uint64_t produced = items[k].bytes() - CSC_PROP_SIZE;
        const uint64_t mb = table_bound(produced, props.csc_blocksize);
        if (mb > 0x7FFFFFFFull) return CSCMI_DEVICE_ERROR;
        const uint8_t *stream = reused(k) ? W.arc + at[k] + CSC_PROP_SIZE : (const uint8_t *)jobs[job_of[k]].dst;
        bj[k] = BlockTableJob{stream, produced, props.csc_blocksize, (uint32_t)mb, slots};
        slots += mb;
    }
    std::vector<BlockTableRes> br;
    std::vector<uint64_t> sizes;
    std::vector<size_t> task(count);
    std::vector<uint8_t> from_base(count);
    for (size_t k = 0; k < count; k++) { task[k] = first + k; from_base[k] = reused(k); }
    rc = dev_block_tables(W, bj, task, from_base, br, sizes);
    if (rc) return rc;

    // 6. the tasks' extents
    size_t nx = 0;
    for (size_t k = 0; k < count; k++) {
        std::vector<Extent> &ext = W.abindex[first + k];
        uint64_t pos = at[k];
        for (uint32_t i = 0; i < br[k].nblocks; i++, nx++) { ext.push_back(Extent{pos, sizes[nx]}); pos += sizes[nx]; }
        if (pos - at[k] != items[k].bytes()) return reused(k) ? -1 : CSCMI_DEVICE_ERROR;
    }
    return 0;
}

// One check wave of CSAMI_DeviceUpdate: candidates cand[first, first + count).  Three launches whatever the mode: k_gather_extents
// (every candidate's 10 property bytes and, where the streams are decoded, those of more than one archive block), the compare
// kernel or the sum pass, and the fold.  A candidate leaves as CSA_UPD_REUSED -- its fragments' checksums those of this pass -- or
// as PROPS, CHANGED or BASE_BAD.  0 or CSCMI_DEVICE_ERROR.
int dev_check_wave(WriteCtx &W, UpdateCtx &U, AddPlan &P, const std::vector<size_t> &cand, size_t first, size_t count)
{
    using namespace csadev;
    // 1. the base streams, staged (under trust: their property bytes alone), and the property bytes back: a candidate whose 10 bytes
    // are not what this call's encoder would write is out
    StagedStreams St;
    for (size_t k = 0; k < count; k++) {
        const UpdTask &u = U.tasks[cand[first + k]];
        St.tasks.push_back(StagedStreams::Task{&u.ext, u.stream, P.tasks[cand[first + k]].total});
    }
    const bool staged = St.stage(U.base->arc, !U.trust, W.tm, &U.ms, U.U.check_launches);
    W.S.upload_bytes += St.table_bytes;
    if (!staged) return CSCMI_DEVICE_ERROR;
    W.S.readback_bytes += CSC_PROP_SIZE * count;
    for (size_t k = 0; k < count; k++) {
        UpdTask &u = U.tasks[cand[first + k]];
        CSCProps want;
        uint8_t wb[CSC_PROP_SIZE];
        CSCEncProps_Init(&want, (uint32_t)std::min<uint64_t>(P.o.dict_size, P.tasks[cand[first + k]].total), P.o.level);
        CSCEnc_WriteProperties(&want, wb, 0);
        if (!St.has_props(k)) { u.candidate = false; u.status = U.trust ? CSA_UPD_PROPS : CSA_UPD_BASE_BAD; }
        else if (memcmp(wb, St.props_of(k), CSC_PROP_SIZE) != 0) { u.candidate = false; u.status = CSA_UPD_PROPS; }
    }

    // 2. verify: the base streams decoded, as CSAMI_DeviceCompareSlices decodes them -- reusable only if the stream decodes, gives
    // exactly the task's bytes and is consumed to its last byte
    if (!U.trust) {
        std::vector<CSCMIDevDecode> jobs;
        std::vector<size_t> job_task;
        for (size_t k = 0; k < count; k++) {
            if (!U.tasks[cand[first + k]].candidate) continue;
            jobs.push_back(St.job(k));
            job_task.push_back(k);
        }
        if (!jobs.empty()) {
            CSCMIDevDecodeStats ds;
            memset(&ds, 0, sizeof(ds));
            if (CSCMI_DecodeDeviceBatch((int)jobs.size(), jobs.data(), NULL, &ds) != 0) return CSCMI_DEVICE_ERROR;
            U.U.decode_launches += ds.launches;
            for (size_t i = 0; i < jobs.size(); i++) {
                if (jobs[i].rc == CSCMI_DEVICE_ERROR) return CSCMI_DEVICE_ERROR;
                UpdTask &u = U.tasks[cand[first + job_task[i]]];
                U.U.decoded_bytes += std::min<uint64_t>(jobs[i].produced, jobs[i].dst_cap);
                if (jobs[i].rc != 0 || jobs[i].produced != jobs[i].dst_cap || jobs[i].consumed != jobs[i].src_size) {
                    u.candidate = false;
                    u.status = CSA_UPD_BASE_BAD;
                }
            }
        }
    }

    // 3. the candidates' fragments: the decoded bytes against the caller's (verify), or the caller's summed where they lie and
    // folded against the base index's checksums (trust)
    FragTables T(U.trust ? FragTables::kGathered : FragTables::kSpread);
    std::vector<FilePiece *> ff_piece;
    std::vector<size_t> ff_task;
    CSADevSpreadStats X;
    CSADevGatherStats G;
    memset(&X, 0, sizeof(X));
    memset(&G, 0, sizeof(G));
    for (size_t k = 0; k < count; k++) {
        const size_t ti = cand[first + k];
        const UpdTask &u = U.tasks[ti];
        if (!u.candidate) continue;
        size_t fi = 0;
        for (FilePiece &f : P.tasks[ti].files) {
            const uint32_t base_sum = u.base_sums[fi++];
            if (!f.size) { f.checksum = 0; continue; }                         // adler32 of nothing, seed 0
            const bool ok = U.trust ? T.add_gathered(W.buf(f), nullptr, W.slice(f), f.off, f.size, G, base_sum)
                                    : T.add_spread(St.raw(k) + f.posblock, (uint8_t *)W.buf(f), W.slice(f), f.off, f.size, 0, f.size, true, X);
            if (!ok) return CSCMI_DEVICE_ERROR;
            ff_piece.push_back(&f);
            ff_task.push_back(ti);
            U.U.checked_bytes += f.size;
        }
    }
    const LaunchSlot slot = {W.tm, &U.ms, &U.ms, U.U.check_launches};
    std::vector<uint8_t> differs(ff_piece.size(), 0);
    if (U.trust) {
        std::vector<FragResult> res;
        if (!T.sum(slot, true, &W.S.upload_bytes, res)) return CSCMI_DEVICE_ERROR;
        W.S.readback_bytes += res.size() * sizeof(FragResult);
        for (size_t i = 0; i < res.size(); i++) { ff_piece[i]->checksum = res[i].adler; differs[i] = !U.digests && !res[i].ok; }
    } else {
        std::vector<FragDiff> rd;
        if (!T.compare(slot, &W.S.upload_bytes, rd)) return CSCMI_DEVICE_ERROR;
        W.S.readback_bytes += rd.size() * sizeof(FragDiff);
        // (where no byte differs the sum of the decoded bytes is the sum of the caller's)
        for (size_t i = 0; i < rd.size(); i++) { ff_piece[i]->checksum = rd[i].adler; differs[i] = rd[i].first < T.frags[i].size; }
    }
    for (size_t i = 0; i < differs.size(); i++)
        if (differs[i]) { UpdTask &u = U.tasks[ff_task[i]]; u.candidate = false; u.status = CSA_UPD_CHANGED; }
    for (size_t k = 0; k < count; k++) {
        UpdTask &u = U.tasks[cand[first + k]];
        if (U.digests && u.candidate && u.digest_changed) { u.candidate = false; u.status = CSA_UPD_CHANGED; }
        if (u.candidate) u.status = CSA_UPD_REUSED;
        else if (U.trust && u.status == CSA_UPD_CHANGED) u.have_sums = true;
        u.candidate = false;
    }
    return 0;
}

// ---- CSAMI_DeviceUpdateInPlace: the new archive takes the base's place in the caller's buffer ----
// Nothing is stored into the buffer before every size is known and the last refusal has passed: the encoded streams are held in
// scratch (dev_hold_wave), the reused ones are walked where they lie in the base (dev_reused_tables), the layout and the index are
// made on the host, and only then the reused streams move (csa_dev_move.h, k_move_extents) and everything else is placed
// (dev_move_and_place).

thread_local double g_move_ms[3] = {0, 0, 0};          // CSAMI_DeviceMoveKernelMs: park, left, right

struct HeldTask {
    const uint8_t *stream = nullptr;           // an encoded task: its stream in held memory, `produced` bytes
    uint64_t produced = 0;
    uint8_t props[CSC_PROP_SIZE];
    std::vector<uint64_t> blocks;              // every task: its archive blocks' sizes
};
struct InPlace {
    uint64_t buf_cap = 0;
    CSADevMoveStats M;
    std::vector<HeldTask> held;                // per task of the plan
    std::list<DevBuf> mem;                     // the held streams, one allocation a wave
    uint64_t held_bytes = 0;
    std::vector<uint64_t> at;                  // where each task's stream will begin
};

// One wave of the update in place: gather, sum and encode as dev_write_wave; the block tables of the encoded streams where they lie
// in scratch; the streams compacted to their `produced` bytes into held memory with one k_gather_extents launch.  The wave's
// oversized scratch goes with E.  At most five launches a wave.  0 or CSCMI_DEVICE_ERROR.
int dev_hold_wave(WriteCtx &W, AddPlan &P, size_t first, size_t count, InPlace &IP)
{
    using namespace csadev;
    WaveStreams E;
    int rc = E.encode(W, P, first, count);
    if (rc || E.jobs.empty()) return rc;
    std::vector<BlockTableJob> bj;
    std::vector<size_t> task;
    uint64_t slots = 0, bytes = 0;
    for (size_t k = 0; k < count; k++) {
        if (E.job_of[k] == SIZE_MAX) continue;
        const CSCMIDevEncode &j = E.jobs[E.job_of[k]];
        const uint64_t mb = table_bound(j.produced, j.props.csc_blocksize);
        if (mb > 0x7FFFFFFFull) return CSCMI_DEVICE_ERROR;
        bj.push_back(BlockTableJob{(const uint8_t *)j.dst, (uint64_t)j.produced, j.props.csc_blocksize, (uint32_t)mb, slots});
        task.push_back(first + k);
        slots += mb;
        bytes += ((uint64_t)j.produced + 15) & ~15ull;
    }
    std::vector<BlockTableRes> br;
    std::vector<uint64_t> sizes;
    rc = dev_block_tables(W, bj, task, std::vector<uint8_t>(bj.size(), 0), br, sizes);
    if (rc) return rc;
    IP.mem.emplace_back();
    if (!IP.mem.back().alloc(bytes)) return CSCMI_DEVICE_ERROR;
    IP.held_bytes += bytes;
    IP.M.held_stream_bytes = std::max<uint64_t>(IP.M.held_stream_bytes, IP.held_bytes);
    std::vector<CopyPiece> gp;
    uint64_t off = 0;
    size_t nx = 0;
    for (size_t i = 0; i < bj.size(); i++) {
        const CSCMIDevEncode &j = E.jobs[E.job_of[task[i] - first]];
        HeldTask &h = IP.held[task[i]];
        h.stream = (const uint8_t *)IP.mem.back().p + off;
        h.produced = j.produced;
        CSCEnc_WriteProperties(&j.props, h.props, 0);                          // csa_worker.cpp:38-42
        uint64_t sum = 0;
        for (uint32_t b = 0; b < br[i].nblocks; b++, nx++) { h.blocks.push_back(sizes[nx]); sum += sizes[nx]; }
        if (sum != CSC_PROP_SIZE + h.produced) return CSCMI_DEVICE_ERROR;
        piece_split((const uint8_t *)j.dst, (uint8_t *)IP.mem.back().p + off, h.produced, kGatherPiece, [&](uint64_t, const CopyPiece &p) { gp.push_back(p); });
        off += (h.produced + 15) & ~15ull;
    }
    DevBuf d_gp;
    if (gp.size() > 0x7FFFFFFFull || !dev_upload(W, d_gp, gp.data(), gp.size() * sizeof(CopyPiece))) return CSCMI_DEVICE_ERROR;
    return W.tm.timed(&g_write_ms[3], W.S.launches, [&] { launch_gather_extents(d_gp.p, (uint32_t)gp.size(), W.tm.st); }) ? 0 : CSCMI_DEVICE_ERROR;
}

// The block tables of the reused streams, walked where they lie in the base: a stream of one base extent in place, one of several
// staged back to back first (one k_gather_extents launch for all of them, as StagedStreams stages them for the read), kTableMaxJobs
// streams a k_block_table launch.  0, CSCMI_DEVICE_ERROR, or -1: a stream does not end at its length.  Only reads the base.
int dev_reused_tables(WriteCtx &W, UpdateCtx &U, AddPlan &P, InPlace &IP)
{
    using namespace csadev;
    std::vector<size_t> R;
    for (size_t i = 0; i < P.tasks.size(); i++) if (U.reused(i)) R.push_back(i);
    if (R.empty()) return 0;
    std::vector<uint64_t> gat_off(R.size(), 0);
    uint64_t gat_bytes = 0;
    std::vector<CopyPiece> gp;
    for (size_t k = 0; k < R.size(); k++) {
        const UpdTask &u = U.tasks[R[k]];
        if (u.stream < CSC_PROP_SIZE) return -1;
        if (u.ext.size() < 2) continue;
        gat_off[k] = gat_bytes;
        gat_bytes += (u.stream - CSC_PROP_SIZE + 255) & ~255ull;
    }
    DevBuf d_gat, d_gp;
    if (gat_bytes) {
        if (!d_gat.alloc(gat_bytes)) return CSCMI_DEVICE_ERROR;
        for (size_t k = 0; k < R.size(); k++) {
            const UpdTask &u = U.tasks[R[k]];
            if (u.ext.size() < 2) continue;
            uint64_t pos = 0;                                                    // position in the task's stream
            for (const Extent &x : u.ext) {
                const uint64_t skip = pos < CSC_PROP_SIZE ? std::min<uint64_t>(CSC_PROP_SIZE - pos, x.size) : 0;
                if (x.size > skip)
                    piece_split(U.base->arc + x.off + skip, (uint8_t *)d_gat.p + gat_off[k] + (pos + skip - CSC_PROP_SIZE), x.size - skip, kGatherPiece,
                                [&](uint64_t, const CopyPiece &p) { gp.push_back(p); });
                pos += x.size;
            }
        }
        if (gp.size() > 0x7FFFFFFFull || !dev_upload(W, d_gp, gp.data(), gp.size() * sizeof(CopyPiece))) return CSCMI_DEVICE_ERROR;
        if (!W.tm.timed(&g_write_ms[3], W.S.launches, [&] { launch_gather_extents(d_gp.p, (uint32_t)gp.size(), W.tm.st); })) return CSCMI_DEVICE_ERROR;
    }
    for (size_t first = 0; first < R.size(); first += kTableMaxJobs) {
        const size_t count = std::min<size_t>(kTableMaxJobs, R.size() - first);
        std::vector<BlockTableJob> bj;
        std::vector<size_t> task;
        uint64_t slots = 0;
        for (size_t k = first; k < first + count; k++) {
            const UpdTask &u = U.tasks[R[k]];
            CSCProps props;                                                      // (the stream's 10 bytes are these props': dev_check_wave)
            CSCEncProps_Init(&props, (uint32_t)std::min<uint64_t>(P.o.dict_size, P.tasks[R[k]].total), P.o.level);
            const uint64_t produced = u.stream - CSC_PROP_SIZE, mb = table_bound(produced, props.csc_blocksize);
            if (mb > 0x7FFFFFFFull) return CSCMI_DEVICE_ERROR;
            const uint8_t *stream = u.ext.size() < 2 ? U.base->arc + u.ext[0].off + CSC_PROP_SIZE : (const uint8_t *)d_gat.p + gat_off[k];
            bj.push_back(BlockTableJob{stream, produced, props.csc_blocksize, (uint32_t)mb, slots});
            task.push_back(R[k]);
            slots += mb;
        }
        std::vector<BlockTableRes> br;
        std::vector<uint64_t> sizes;
        const int rc = dev_block_tables(W, bj, task, std::vector<uint8_t>(count, 1), br, sizes);
        if (rc) return rc;
        size_t nx = 0;
        for (size_t i = 0; i < count; i++) {
            HeldTask &h = IP.held[task[i]];
            uint64_t sum = 0;
            for (uint32_t b = 0; b < br[i].nblocks; b++, nx++) { h.blocks.push_back(sizes[nx]); sum += sizes[nx]; }
            if (sum != U.tasks[task[i]].stream) return -1;
        }
    }
    return 0;
}

// One phase of the moves: the chunk table up, the state block zeroed, the launch, the error word back.
int dev_move_phase(WriteCtx &W, const std::vector<csadev::MoveChunk> &chunks, DevBuf &d_chunks, DevBuf &d_state, size_t state_bytes, InPlace &IP, double *ms)
{
    uint32_t state[csadev::kMoveStateWords] = {0, 0, 0, 0};
    const double before = *ms;
    if (!W.tm.timed(ms, IP.M.launches, [&] {
            launch_move_extents(d_chunks.p, (uint32_t)chunks.size(), W.arc, IP.buf_cap, d_state.p, state_bytes, W.tm.st); })) return CSCMI_DEVICE_ERROR;
    IP.M.kernel_ms += *ms - before;
    if (!HIP_OK(hipMemcpy(state, d_state.p, sizeof(state), hipMemcpyDeviceToHost))) return CSCMI_DEVICE_ERROR;
    if (state[1]) {
        fprintf(stderr, "csa-mi355x: k_move_extents: ticket %u gave up waiting for the chunks in front of it\n", state[1] - 1);
        return CSCMI_DEVICE_ERROR;
    }
    return 0;
}

// The last refusal, then the stores: WRITE_ERROR with the buffer untouched if header, streams and index pass buf_cap; else the
// reused streams move to their places (park, left phase, right phase) and one k_gather_extents launch places the held streams with
// their property bytes, the parked streams, the index stream `job` and the header.  Every table and every byte of scratch is
// there before the first launch, so that from then on only a failing launch can end the call.
int dev_move_and_place(WriteCtx &W, UpdateCtx &U, AddPlan &P, InPlace &IP, const CSCMIDevEncode &job, const uint8_t *hdr)
{
    using namespace csadev;
    uint64_t end;
    if (!add_ok(W.arc_end, CSC_PROP_SIZE + (uint64_t)job.produced, &end) || end > IP.buf_cap) return WRITE_ERROR;
    std::vector<Move> moves;
    for (size_t i = 0; i < P.tasks.size(); i++) {
        if (!U.reused(i)) continue;
        uint64_t d = IP.at[i];
        for (const Extent &x : U.tasks[i].ext) { moves.push_back(Move{x.off, d, x.size}); d += x.size; }
    }
    MovePlan MP;
    plan_moves(moves, MP);
    if (MP.phase[0].size() > 0x7FFFFFFFull || MP.phase[1].size() > 0x7FFFFFFFull) return CSCMI_DEVICE_ERROR;
    IP.M.moves = MP.moves; IP.M.moved_bytes = MP.moved_bytes; IP.M.parked_moves = MP.parked_moves; IP.M.parked_bytes = MP.parked_bytes;
    // scratch and tables
    DevBuf d_park, d_pp, d_chunks[2], d_state, d_host, d_gp;
    std::vector<CopyPiece> pp, gp;
    std::vector<uint64_t> park_off;
    uint64_t park_bytes = 0;
    for (const Move &m : MP.parked) { park_off.push_back(park_bytes); park_bytes += (m.len + 15) & ~15ull; }
    if (park_bytes && !d_park.alloc(park_bytes)) return CSCMI_DEVICE_ERROR;
    auto put = [&](uint64_t, const CopyPiece &p) { gp.push_back(p); };
    for (size_t k = 0; k < MP.parked.size(); k++) {
        piece_split(W.arc + MP.parked[k].src, (uint8_t *)d_park.p + park_off[k], MP.parked[k].len, kGatherPiece, [&](uint64_t, const CopyPiece &p) { pp.push_back(p); });
        piece_split((const uint8_t *)d_park.p + park_off[k], W.arc + MP.parked[k].dst, MP.parked[k].len, kGatherPiece, put);
    }
    // the bytes that come from the host: the header and the property bytes of every encoded stream and of the index stream
    std::vector<uint8_t> host(hdr, hdr + kHeaderSize);
    for (size_t i = 0; i < P.tasks.size(); i++)
        if (!U.reused(i)) host.insert(host.end(), IP.held[i].props, IP.held[i].props + CSC_PROP_SIZE);
    uint8_t iprops[CSC_PROP_SIZE];
    CSCEnc_WriteProperties(&job.props, iprops, 0);
    host.insert(host.end(), iprops, iprops + CSC_PROP_SIZE);
    if (!dev_upload(W, d_host, host.data(), host.size())) return CSCMI_DEVICE_ERROR;
    gp.push_back(CopyPiece{(const uint8_t *)d_host.p, W.arc, (uint32_t)kHeaderSize, 0});
    uint64_t hp = kHeaderSize;
    for (size_t i = 0; i < P.tasks.size(); i++) {
        if (U.reused(i)) continue;
        gp.push_back(CopyPiece{(const uint8_t *)d_host.p + hp, W.arc + IP.at[i], CSC_PROP_SIZE, 0});
        piece_split(IP.held[i].stream, W.arc + IP.at[i] + CSC_PROP_SIZE, IP.held[i].produced, kGatherPiece, put);
        hp += CSC_PROP_SIZE;
    }
    gp.push_back(CopyPiece{(const uint8_t *)d_host.p + hp, W.arc + W.arc_end, CSC_PROP_SIZE, 0});
    piece_split((const uint8_t *)job.dst, W.arc + W.arc_end + CSC_PROP_SIZE, job.produced, kGatherPiece, put);
    if (gp.size() > 0x7FFFFFFFull || pp.size() > 0x7FFFFFFFull || !dev_upload(W, d_gp, gp.data(), gp.size() * sizeof(CopyPiece))
        || (!pp.empty() && !dev_upload(W, d_pp, pp.data(), pp.size() * sizeof(CopyPiece)))) return CSCMI_DEVICE_ERROR;
    const size_t nflags = std::max(MP.phase[0].size(), MP.phase[1].size());
    const size_t state_bytes = ((kMoveStateWords + nflags) * sizeof(uint32_t) + 15) & ~(size_t)15;
    for (int ph = 0; ph < 2; ph++)
        if (!MP.phase[ph].empty() && !dev_upload(W, d_chunks[ph], MP.phase[ph].data(), MP.phase[ph].size() * sizeof(MoveChunk))) return CSCMI_DEVICE_ERROR;
    if (nflags && !d_state.alloc(state_bytes)) return CSCMI_DEVICE_ERROR;
    // ---- from here on the buffer is written
    if (!pp.empty()) {
        const double before = g_move_ms[0];
        if (!W.tm.timed(&g_move_ms[0], IP.M.launches, [&] { launch_gather_extents(d_pp.p, (uint32_t)pp.size(), W.tm.st); })) return CSCMI_DEVICE_ERROR;
        IP.M.kernel_ms += g_move_ms[0] - before;
    }
    for (int ph = 0; ph < 2; ph++) {
        if (MP.phase[ph].empty()) continue;
        const int rc = dev_move_phase(W, MP.phase[ph], d_chunks[ph], d_state, state_bytes, IP, &g_move_ms[1 + ph]);
        if (rc) return rc;
    }
    if (!W.tm.timed(&g_write_ms[3], W.S.launches, [&] { launch_gather_extents(d_gp.p, (uint32_t)gp.size(), W.tm.st); })) return CSCMI_DEVICE_ERROR;
    W.arc_end = end;
    return 0;
}

// What the write, the update and CSAMI_DeviceDigestSlices refuse in the caller's sources (-1): the slices, each inside its buffer and
// selecting exactly its entry's bytes; sl[i] is entry i's checked slice, and hull[i] / hull_size[i] its hull, which is all that is
// loaded (slices == NULL: every entry whole -- all of a buffer of esize bytes).  G gets the selected and the hull bytes.
int check_sources(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, const CSADevFile *files, uint32_t n_files,
                  std::vector<csadev::Slice> &sl, std::vector<const void *> &hull, std::vector<uint64_t> &hull_size, CSADevGatherStats &G)
{
    sl.assign(n_files, csadev::Slice{0, 0, 0, 0});
    hull.assign(n_files, nullptr);
    hull_size.assign(n_files, 0);
    for (uint32_t i = 0; i < n_files; i++) {
        const uint64_t esize = (uint64_t)files[i].esize;                     // (plan_write: not negative)
        sl[i] = slices ? dev_slice(slices[i]) : whole_slice(esize);
        uint64_t bytes, at;
        if (!csadev::slice_check(sl[i], slices ? sizes[i] : esize, &bytes) || bytes != esize) return -1;
        if (!sl[i].count) continue;
        if (!ptrs[i] || !add_ok((uintptr_t)ptrs[i], sl[i].offset, &at)) return -1;
        hull[i] = (const void *)(uintptr_t)at;
        hull_size[i] = (sl[i].count - 1) * sl[i].stride + sl[i].run;         // (checked by slice_check)
        G.selected_bytes += bytes;                                           // (plan_write: the sizes sum to at most 2^60)
        if (!add_ok(G.hull_bytes, hull_size[i], &G.hull_bytes)) return -1;
    }
    return 0;
}

// Where each fragment of the plan will stand in the index the write packs -- the entries in name order, an entry's fragments in the
// order the tasks hand them out (csarc.cpp:371-386) -- and so in the digest table: place[task][piece].  Returns their number.
uint64_t plan_frag_places(AddPlan &P, std::vector<std::vector<uint64_t>> &place)
{
    std::map<const Entry *, uint64_t> count, first;
    for (const Task &t : P.tasks)
        for (const FilePiece &f : t.files) count[&f.it->second]++;
    uint64_t n = 0;
    for (const auto &kv : P.index) { first[&kv.second] = n; n += count[&kv.second]; }
    place.assign(P.tasks.size(), std::vector<uint64_t>());
    for (size_t ti = 0; ti < P.tasks.size(); ti++)
        for (const FilePiece &f : P.tasks[ti].files) place[ti].push_back(first[&f.it->second]++);
    return n;
}

// The digest pass of a write, an update or CSAMI_DeviceDigestSlices: with `all`, every fragment of the plan where it lies in the
// caller's buffers, its digest to out[place] (out == NULL: nowhere); else the candidates' alone.  A candidate's fragments are compared
// with `expect` at their places in the base index (U == NULL or expect == NULL: nothing is compared), and a candidate one of whose
// fragments differs is marked.  0 or CSCMI_DEVICE_ERROR.
int dev_digest_plan(AddPlan &P, const void *const *ptrs, const csadev::Slice *slices, const std::vector<std::vector<uint64_t>> &place, bool all,
                    UpdateCtx *U, DevTimer &tm, DigestCall &dg)
{
    DigestPass DP;
    std::vector<size_t> ff_task;
    for (size_t ti = 0; ti < P.tasks.size(); ti++) {
        const bool compared = U && dg.expect && U->tasks[ti].candidate;
        if (!all && !compared) continue;
        size_t fi = 0;
        for (const FilePiece &f : P.tasks[ti].files) {
            const uint32_t row = f.it->second.row;
            if (!DP.add((const uint8_t *)ptrs[row], slices[row], f.off, f.size, place[ti][fi], compared ? U->tasks[ti].base_pos[fi] : csadev::kDigestNone))
                return CSCMI_DEVICE_ERROR;
            ff_task.push_back(ti);
            fi++;
        }
    }
    std::vector<uint32_t> differs;
    if (!DP.run(tm, dg.out, dg.expect, dg.ds, differs)) return CSCMI_DEVICE_ERROR;
    for (size_t i = 0; i < differs.size(); i++)
        if (differs[i]) U->tasks[ff_task[i]].digest_changed = true;
    return 0;
}

}   // namespace

extern "C" {

int CSAMI_DeviceWriteFragCount(const CSADevFile *files, uint32_t n_files, const char *arcname, const CSAOptions *opt, uint64_t *n_frags)
{
    (void)arcname;
    AddPlan P;
    const int rc = plan_write(P, files, n_files, opt, nullptr);
    if (rc == -1) return -1;
    uint64_t n = 0;
    for (const Task &t : P.tasks) n += t.files.size();
    if (n_frags) *n_frags = n;
    return rc;
}

int CSAMI_DeviceDigestSlices(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, const CSADevFile *files, uint32_t n_files,
                             const char *arcname, const CSAOptions *opt, CSADevDigest *digests_out, uint64_t digests_cap, CSADevDigestStats *ds)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    DigestCall dg = {digests_out, nullptr, CSADevDigestStats()};
    memset(&dg.ds, 0, sizeof(dg.ds));
    g_digest_ms[0] = g_digest_ms[1] = 0;
    if (ds) *ds = dg.ds;
    if (!arcname || (n_files && (!ptrs || !files || !sizes != !slices))) return -1;
    AddPlan P;
    int rc = plan_write(P, files, n_files, opt, nullptr);
    if (rc) return rc;
    std::vector<csadev::Slice> sl;
    std::vector<const void *> hull;
    std::vector<uint64_t> hull_size;
    std::vector<std::vector<uint64_t>> place;
    CSADevGatherStats G;
    memset(&G, 0, sizeof(G));
    if (check_sources(ptrs, sizes, slices, files, n_files, sl, hull, hull_size, G) != 0) return -1;
    const uint64_t n_frags = plan_frag_places(P, place);
    if ((n_frags && !digests_out) || CSAMI_CheckBuffers(hull.data(), hull_size.data(), n_files, digests_out, n_frags * sizeof(CSADevDigest), 0, nullptr) != 0)
        return -1;
    if (digests_cap < n_frags) return WRITE_ERROR;
    DevTimer tm;
    if (!tm.ok) return CSCMI_DEVICE_ERROR;
    dg.ds.first_mismatch = UINT64_MAX;
    rc = dev_digest_plan(P, ptrs, sl.data(), place, true, nullptr, tm, dg);
    if (ds) *ds = dg.ds;
    return rc;
}

int CSAMI_DeviceWritePlan(const CSADevFile *files, uint32_t n_files, const char *arcname, const CSAOptions *opt,
                          uint32_t *n_tasks, uint32_t *max_frags, uint64_t *raw_bytes)
{
    (void)arcname;
    AddPlan P;
    uint64_t raw = 0;
    const int rc = plan_write(P, files, n_files, opt, &raw);
    if (rc == -1) return -1;
    std::map<const void *, uint32_t> nfr;
    uint32_t mx = 0;
    for (const Task &t : P.tasks)
        for (const FilePiece &f : t.files) mx = std::max(mx, ++nfr[(const void *)&*f.it]);
    if (n_tasks) *n_tasks = (uint32_t)P.tasks.size();
    if (max_frags) *max_frags = mx;
    if (raw_bytes) *raw_bytes = raw;
    return rc;
}

int CSAMI_DeviceWrite(const void *src_dev, uint64_t src_size, CSADevFile *files, uint32_t n_files, const char *arcname,
                      void *arc_dev, uint64_t arc_cap, const CSAOptions *opt, CSADevWriteStats *st)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    if (st) memset(st, 0, sizeof(*st));
    for (double &m : g_write_ms) m = 0;
    // ---- what only this call can refuse: the entries against src_size, and src as a whole against arc
    const uintptr_t s0 = (uintptr_t)src_dev, a0 = (uintptr_t)arc_dev;
    uint64_t s1, a1;
    if (!arcname || (!src_dev && src_size) || (!arc_dev && arc_cap) || !add_ok(s0, src_size, &s1) || !add_ok(a0, arc_cap, &a1)) return -1;
    if (src_size && arc_cap && s0 < a1 && a0 < s1) return -1;
    if (n_files && !files) return -1;
    std::vector<const void *> ptrs(n_files, nullptr);
    for (uint32_t i = 0; i < n_files; i++) {
        uint64_t end;
        if (files[i].esize < 0 || !add_ok(files[i].offset, (uint64_t)files[i].esize, &end) || end > src_size) return -1;
        if (files[i].esize) ptrs[i] = (const uint8_t *)src_dev + files[i].offset;
    }
    return CSAMI_DeviceWriteFrom(ptrs.data(), files, n_files, arcname, arc_dev, arc_cap, opt, st);
}

int CSAMI_DeviceWriteFrom(const void *const *ptrs, CSADevFile *files, uint32_t n_files, const char *arcname,
                          void *arc_dev, uint64_t arc_cap, const CSAOptions *opt, CSADevWriteStats *st)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    // every entry whole: the update reads sizes == slices == NULL as that (a table the write refuses is refused there)
    return CSAMI_DeviceUpdate(nullptr, ptrs, nullptr, nullptr, files, n_files, arcname, arc_dev, arc_cap, 0, opt, st, nullptr, nullptr, nullptr, 0);
}

int CSAMI_DeviceWriteSlices(const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, CSADevFile *files, uint32_t n_files,
                            const char *arcname, void *arc_dev, uint64_t arc_cap, const CSAOptions *opt, CSADevWriteStats *st,
                            CSADevGatherStats *gather_stats)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    if (n_files && (!sizes || !slices)) {                                    // (the update reads "both NULL" as "every entry whole")
        if (st) memset(st, 0, sizeof(*st));
        if (gather_stats) memset(gather_stats, 0, sizeof(*gather_stats));
        for (double &m : g_write_ms) m = 0;
        return -1;
    }
    return CSAMI_DeviceUpdate(nullptr, ptrs, sizes, slices, files, n_files, arcname, arc_dev, arc_cap, 0, opt, st, gather_stats, nullptr, nullptr, 0);
}

int CSAMI_DeviceUpdate(CSADevArchive *base, const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, CSADevFile *files,
                       uint32_t n_files, const char *arcname, void *arc_dev, uint64_t arc_cap, uint32_t flags, const CSAOptions *opt,
                       CSADevWriteStats *st, CSADevGatherStats *gather_stats, CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks,
                       uint32_t task_cap)
{
    return CSAMI_DeviceUpdateDigests(base, nullptr, 0, ptrs, sizes, slices, files, n_files, arcname, arc_dev, arc_cap, flags, opt, st, gather_stats,
                                     update_stats, tasks, task_cap, nullptr, 0, nullptr);
}

// CSAMI_DeviceUpdateDigests, and with `ip` CSAMI_DeviceUpdateInPlace: the same refusals, plan, candidates, digest pass, check waves
// and index; what differs is where the streams go, and when (arc_dev and arc_cap are then the base's buffer and ip->buf_cap).
static int dev_update(CSADevArchive *base, const CSADevDigest *base_digests, uint64_t n_base_digests, const void *const *ptrs,
                      const uint64_t *sizes, const CSADevSlice *slices, CSADevFile *files, uint32_t n_files, const char *arcname,
                      void *arc_dev, uint64_t arc_cap, uint32_t flags, const CSAOptions *opt, CSADevWriteStats *st,
                      CSADevGatherStats *gather_stats, CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks, uint32_t task_cap,
                      CSADevDigest *digests_out, uint64_t digests_cap, CSADevDigestStats *ds, InPlace *ip)
{
    const double t0 = now_s();
    WriteCtx W;
    UpdateCtx U;
    DigestCall dg = {digests_out, base_digests, CSADevDigestStats()};
    memset(&W.S, 0, sizeof(W.S));
    memset(&W.G, 0, sizeof(W.G));
    memset(&U.U, 0, sizeof(U.U));
    memset(&dg.ds, 0, sizeof(dg.ds));
    g_digest_ms[0] = g_digest_ms[1] = 0;
    if (st) *st = W.S;
    if (gather_stats) *gather_stats = W.G;
    if (update_stats) *update_stats = U.U;
    if (ds) *ds = dg.ds;
    for (double &m : g_write_ms) m = 0;
    // ---- everything the host can refuse, before any launch
    uint64_t a1;
    if (!arcname || (!arc_dev && arc_cap) || !add_ok((uintptr_t)arc_dev, arc_cap, &a1) || (n_files && (!ptrs || !files || !sizes != !slices))) return -1;
    if (ip && !base) return -1;
    AddPlan P;
    int rc = plan_write(P, files, n_files, opt, &W.S.raw_bytes);
    if (rc) return rc;
    // the slices, each inside its buffer and selecting exactly its entry's bytes; the hulls, which are all that is loaded
    // (slices == NULL: every entry whole -- all of a buffer of esize bytes)
    std::vector<csadev::Slice> sl;
    std::vector<const void *> hull;
    std::vector<uint64_t> hull_size;
    CSADevGatherStats G = W.G;
    if (check_sources(ptrs, sizes, slices, files, n_files, sl, hull, hull_size, G) != 0) return -1;
    if (CSAMI_CheckBuffers(hull.data(), hull_size.data(), n_files, arc_dev, arc_cap, 0, nullptr) != 0) return -1;
    if (ip && arc_cap < base->arc_size) return -1;
    if (!ip && base && arc_cap && base->arc_size) {                          // the base is read while arc is written: CSAMI_DeviceUpdateInPlace is the call for that
        const uint64_t b0 = (uint64_t)(uintptr_t)base->arc, x0 = (uint64_t)(uintptr_t)arc_dev;
        if (x0 <= b0 + (base->arc_size - 1) && b0 <= x0 + (arc_cap - 1)) return -1;
    }
    // the digest tables: the flags, the base table's length, and where the two lie
    std::vector<std::vector<uint64_t>> place;
    const uint64_t n_frags = plan_frag_places(P, place);
    const uint64_t out_bytes = digests_out ? n_frags * sizeof(CSADevDigest) : 0, base_bytes = base_digests ? n_base_digests * sizeof(CSADevDigest) : 0;
    U.digests = (flags & CSAMI_UPDATE_TRUST_DIGESTS) != 0;
    if (U.digests && ((flags & CSAMI_UPDATE_TRUST_SUMS) || !base_digests)) return -1;
    if (base && base_digests) {
        uint64_t nb = 0;
        for (const auto &kv : base->index) nb += kv.second.frags.size();
        if (n_base_digests != nb) return -1;
    }
    for (int k = 0; k < 2; k++) {
        const void *tp = k ? (const void *)base_digests : (const void *)digests_out;
        const uint64_t tb = k ? base_bytes : out_bytes;
        if (!tb) continue;
        if (ranges_meet(tp, tb, arc_dev, arc_cap) || (base && ranges_meet(tp, tb, base->arc, base->arc_size))
            || CSAMI_CheckBuffers(hull.data(), hull_size.data(), n_files, tp, tb, 0, nullptr) != 0) return -1;
    }
    if (ranges_meet(digests_out, out_bytes, base_digests, base_bytes)) return -1;
    if (arc_cap < kHeaderSize || (digests_out && digests_cap < n_frags)) return WRITE_ERROR;
    dg.ds.first_mismatch = UINT64_MAX;
    if (const char *e = getenv("CSA_DEVWRITE_SLACK")) { W.slack = (int64_t)strtoull(e, nullptr, 10); if (W.slack < 0) W.slack = -1; }
    W.ptrs = ptrs; W.slices = sl.data(); W.arc = (uint8_t *)arc_dev; W.arc_cap = arc_cap;
    W.G = G;
    if (!W.tm.ok) return CSCMI_DEVICE_ERROR;

    size_t mem_free = 0, mem_total = 0;
    if (!HIP_OK(hipMemGetInfo(&mem_free, &mem_total))) return CSCMI_DEVICE_ERROR;
    const uint64_t budget = hbm_budget(P.o, mem_free);

    // ---- the update: which tasks of the plan are a task of the base (host), and whether their bytes are still the base's (check waves)
    if (base) {
        const double tc = now_s();
        W.upd = &U;
        U.base = base;
        U.trust = (flags & (CSAMI_UPDATE_TRUST_SUMS | CSAMI_UPDATE_TRUST_DIGESTS)) != 0;
        U.tasks.resize(P.tasks.size());
        std::vector<uint64_t> bids;
        std::vector<std::vector<uint32_t>> sums;
        std::vector<std::vector<uint64_t>> pos;
        U.U.candidates = update_candidates(base->index, P, bids, sums, &pos);
        static const std::vector<Extent> kNoBlocks;
        std::vector<size_t> cand;
        for (size_t i = 0; i < P.tasks.size(); i++) {
            if (bids[i] == UINT64_MAX) continue;
            UpdTask &u = U.tasks[i];
            u.base_bid = bids[i];
            u.candidate = true;
            u.base_sums.swap(sums[i]);
            u.base_pos.swap(pos[i]);
            auto ab = base->abindex.find(bids[i]);
            if (!dev_stream_extents(ab == base->abindex.end() ? kNoBlocks : ab->second, base->arc_size, u.ext, u.stream)) return CSCMI_DEVICE_ERROR;
            cand.push_back(i);
        }
        // the digest pass: every fragment of the plan for the table this call hands out, the candidates' against the base table
        if (digests_out || U.digests) {
            if (!U.digests) dg.expect = nullptr;
            rc = dev_digest_plan(P, ptrs, sl.data(), place, digests_out != nullptr, &U, W.tm, dg);
        }
        // waves as CSAMI_DeviceRead sizes them (a wave that only sums holds no decoder and no scratch)
        const size_t cwidth = P.o.device_streams > 0 ? (size_t)P.o.device_streams : std::max<size_t>(cand.size(), 1);
        for (size_t first = 0; rc == 0 && first < cand.size();) {
            const size_t count = wave_count(first, cand.size(), cwidth, budget, [&](size_t c) {
                if (U.trust) return (uint64_t)0;
                const uint64_t raw = P.tasks[cand[c]].total;
                uint64_t need = decoder_need(raw);
                if (!add_ok(need, raw, &need) || !add_ok(need, U.tasks[cand[c]].stream, &need)) need = UINT64_MAX;
                return need;
            });
            rc = dev_check_wave(W, U, P, cand, first, count);
            U.U.check_waves++;
            first += count;
        }
        U.U.check_kernel_ms = U.ms;
        U.U.seconds_check = now_s() - tc;
    } else if (digests_out) {
        dg.expect = nullptr;
        rc = dev_digest_plan(P, ptrs, sl.data(), place, true, nullptr, W.tm, dg);
    }

    // ---- waves of consecutive task ids, largest first (csarc.cpp:355): the plan's order and the archive's
    size_t width = P.o.device_streams > 0 ? (size_t)P.o.device_streams : csadev::kTableMaxJobs;
    width = std::min<size_t>(width, csadev::kTableMaxJobs);
    if (ip) ip->held.resize(P.tasks.size());
    for (size_t first = 0; rc == 0 && first < P.tasks.size();) {
        // what the task's encoder holds (as encode_tasks reckons), a gathered copy of its input (at most) and its scratch stream;
        // a reused task holds nothing
        const size_t count = wave_count(first, P.tasks.size(), width, budget, [&](size_t i) {
            const Task &t = P.tasks[i];
            if (W.upd && U.reused(i)) return (uint64_t)0;
            CSCProps p;
            CSCEncProps_Init(&p, (uint32_t)std::min<uint64_t>(P.o.dict_size, t.total), P.o.level);
            return (uint64_t)(CSCEnc_EstMemUsage(&p) + (24ull << 20) + t.total + stream_cap(W, t.total));
        });
        rc = ip ? dev_hold_wave(W, P, first, count, *ip) : dev_write_wave(W, P, first, count);
        W.S.waves++;
        for (size_t k = first; k < first + count; k++) { W.S.tasks++; W.S.frags += P.tasks[k].files.size(); }
        first += count;
    }
    // in place: the reused streams' tables where they lie in the base, then -- every size is known -- the layout
    if (ip && rc == 0) rc = dev_reused_tables(W, U, P, *ip);
    if (ip && rc == 0) {
        for (size_t i = 0; i < P.tasks.size(); i++) {
            ip->at.push_back(W.arc_end);
            std::vector<Extent> &ext = W.abindex[i];
            for (uint64_t n : ip->held[i].blocks) { ext.push_back(Extent{W.arc_end, n}); W.arc_end += n; }
        }
    }
    for (size_t i = 0; W.upd && i < P.tasks.size(); i++) {
        const UpdTask &u = U.tasks[i];
        if (u.status == CSA_UPD_REUSED) { U.U.reused_tasks++; U.U.reused_raw_bytes += P.tasks[i].total; U.U.reused_stream_bytes += u.stream; }
        else { U.U.encoded_tasks++; U.U.encoded_raw_bytes += P.tasks[i].total; }
        if (tasks && i < task_cap) tasks[i] = CSADevUpdateTask{u.base_bid, u.status, 0};
    }

    // ---- fragments, index stream, header: csarc.cpp:371-386, 219-288
    if (rc == 0) {
        for (size_t ti = 0; ti < P.tasks.size(); ti++)
            for (const FilePiece &f : P.tasks[ti].files)
                f.it->second.frags.push_back(CSAFrag{(uint32_t)ti, f.checksum, f.posblock, f.size, f.off});
        const std::vector<uint8_t> raw = pack_index(P.index, W.abindex, arcname);
        DevBuf d_raw, d_scr;
        std::list<DevBuf> more;
        std::vector<CSCMIDevEncode> job(1);
        memset(&job[0], 0, sizeof(job[0]));
        CSCEncProps_Init(&job[0].props, 256 * 1024, 2);                      // csarc.cpp:251
        if (raw.size() > 0xFFFFFFFFull) rc = WRITE_ERROR;                    // (the header has 32 bits for it)
        else if (!dev_upload(W, d_raw, raw.data(), raw.size()) || !d_scr.alloc(stream_cap(W, raw.size()))) rc = CSCMI_DEVICE_ERROR;
        if (rc == 0) {
            job[0].src = d_raw.p; job[0].src_size = raw.size();
            job[0].dst = d_scr.p; job[0].dst_cap = (size_t)stream_cap(W, raw.size());
            rc = dev_encode(W, job, more);
        }
        const uint64_t csize = CSC_PROP_SIZE + (uint64_t)job[0].produced;
        if (rc == 0 && csize > 0xFFFFFFFFull) rc = WRITE_ERROR;
        if (rc == 0) {
            uint8_t hdr[kHeaderSize];                                        // csarc.cpp:268-287
            hdr[0] = 'C'; hdr[1] = 'S'; hdr[2] = 'A'; hdr[7] = '1';
            store_le(hdr + 3, kMagicNum, 4);
            store_le(hdr + 8, W.arc_end, 8);
            store_le(hdr + 16, csize, 4);
            store_le(hdr + 20, raw.size(), 4);
            rc = ip ? dev_move_and_place(W, U, P, *ip, job[0], hdr) : dev_place(W, std::vector<Placed>(1, Placed{&job[0], nullptr, nullptr, 0}), hdr);
        }
        if (rc == 0 && ip) {                                                 // the handle describes the new archive, as CSAMI_DeviceOpen would
            Index index;
            BlockIndex abindex;
            std::map<uint64_t, uint64_t> task_raw;
            if (!unpack_index(index, abindex, raw.data(), raw.size()) || !dev_task_sizes(index, task_raw)) rc = CSCMI_DEVICE_ERROR;
            else {
                base->index.swap(index); base->abindex.swap(abindex); base->task_raw.swap(task_raw);
                base->arc_size = W.arc_end;
                base->open_readback = kHeaderSize + CSC_PROP_SIZE + raw.size();
            }
        }
        if (rc == 0) {
            W.S.index_raw_size = raw.size();
            W.S.index_compressed_size = csize;
            W.S.archive_bytes = W.arc_end;
            W.S.n_entries = (uint32_t)P.index.size();
            for (const auto &kv : P.index) {
                files[kv.second.row].size = (uint64_t)kv.second.esize;
                files[kv.second.row].nfrags = (uint32_t)kv.second.frags.size();
            }
        }
    }
    W.S.kernel_ms = g_write_ms[0] + g_write_ms[1] + g_write_ms[2] + g_write_ms[3];
    W.S.seconds_total = now_s() - t0;
    if (st) *st = W.S;
    if (gather_stats) *gather_stats = W.G;
    if (update_stats) *update_stats = U.U;
    if (ds) *ds = dg.ds;
    return rc;
}

int CSAMI_DeviceUpdateDigests(CSADevArchive *base, const CSADevDigest *base_digests, uint64_t n_base_digests, const void *const *ptrs,
                              const uint64_t *sizes, const CSADevSlice *slices, CSADevFile *files, uint32_t n_files, const char *arcname,
                              void *arc_dev, uint64_t arc_cap, uint32_t flags, const CSAOptions *opt, CSADevWriteStats *st,
                              CSADevGatherStats *gather_stats, CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks, uint32_t task_cap,
                              CSADevDigest *digests_out, uint64_t digests_cap, CSADevDigestStats *ds)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    return dev_update(base, base_digests, n_base_digests, ptrs, sizes, slices, files, n_files, arcname, arc_dev, arc_cap, flags, opt, st, gather_stats,
                      update_stats, tasks, task_cap, digests_out, digests_cap, ds, nullptr);
}

int CSAMI_DeviceUpdateInPlace(CSADevArchive *base, uint64_t buf_cap, const CSADevDigest *base_digests, uint64_t n_base_digests,
                              const void *const *ptrs, const uint64_t *sizes, const CSADevSlice *slices, CSADevFile *files, uint32_t n_files,
                              const char *arcname, uint32_t flags, const CSAOptions *opt, CSADevWriteStats *st, CSADevGatherStats *gather_stats,
                              CSADevUpdateStats *update_stats, CSADevUpdateTask *tasks, uint32_t task_cap, CSADevDigest *digests_out,
                              uint64_t digests_cap, CSADevDigestStats *ds, CSADevMoveStats *ms)
{
    if (CSCMI_DeviceCheck() != 0) return CSCMI_DEVICE_ERROR;
    InPlace IP;
    IP.buf_cap = buf_cap;
    memset(&IP.M, 0, sizeof(IP.M));
    for (double &m : g_move_ms) m = 0;
    if (ms) *ms = IP.M;
    // (without a base there is no buffer: the statistics are zeroed as dev_update zeroes them on every refusal)
    const int rc = dev_update(base, base_digests, n_base_digests, ptrs, sizes, slices, files, n_files, arcname, base ? const_cast<uint8_t *>(base->arc) : nullptr,
                              base ? buf_cap : 0, flags, opt, st, gather_stats, update_stats, tasks, task_cap, digests_out, digests_cap, ds, &IP);
    if (ms) *ms = IP.M;
    return rc;
}

void CSAMI_DeviceMoveKernelMs(double ms[3])
{
    for (int i = 0; i < 3; i++) ms[i] = g_move_ms[i];
}

int CSAMI_PlanDeviceUpdate(const uint8_t *raw_index, uint64_t raw_size, uint64_t arc_size, const CSADevFile *files, uint32_t n_files,
                           const CSAOptions *opt, uint64_t *base_bids, uint32_t cap, uint32_t *n_tasks, uint32_t *n_candidates)
{
    Index index;
    DevLayout L;
    if (!dev_plan_strict(raw_index, raw_size, arc_size, nullptr, 0, index, L)) return -1;
    AddPlan P;
    const int rc = plan_write(P, files, n_files, opt, nullptr);
    if (rc) return rc;
    std::vector<uint64_t> bids;
    std::vector<std::vector<uint32_t>> sums;
    const uint32_t n = update_candidates(index, P, bids, sums);
    for (size_t i = 0; base_bids && i < bids.size() && i < cap; i++) base_bids[i] = bids[i];
    if (n_tasks) *n_tasks = (uint32_t)bids.size();
    if (n_candidates) *n_candidates = n;
    return 0;
}

void CSAMI_DeviceWriteKernelMs(double ms[4])
{
    for (int i = 0; i < 4; i++) ms[i] = g_write_ms[i];
}

}   // extern "C"
