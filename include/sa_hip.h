/*
 * sa_hip.h -- C ABI of libsa_hip.so: MI355X (gfx950) suffix-array construction and batched
 * substring query.  Plain C types only; no C++, HIP or torch types cross this boundary
 * (device pointers and the stream travel as void*).
 *
 * Each entry point names the reference interface it replaces (paths relative to the
 * reference repository jdm365/SuffixArray @ 2024_10_08).  INTEGRATION.md shows the
 * reference-side binding (Cython `cdef extern`, Makefile link line).
 *
 * Error convention: libsais' (libsais.h:82-94) -- 0 ok, -1 invalid arguments, -2 out of
 * (host or device) memory; additionally -3 HIP runtime / no usable device, -4 internal
 * device-side failure (bounded spin expired).  Nothing here calls exit() or prints.
 * sa_hip_last_error() returns a thread-local message for the last non-zero return.
 *
 * Threading: every function may be called without the GIL.  A handle owns one HIP stream;
 * calls on the same handle are serialised by an internal mutex; different handles are
 * independent.  The libsais-/engine-compatible wrappers create a private handle per call.
 */
#ifndef SA_HIP_H
#define SA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_HIP_OK            0
#define SA_HIP_EINVAL       (-1)
#define SA_HIP_ENOMEM       (-2)
#define SA_HIP_EHIP         (-3)
#define SA_HIP_EINTERNAL    (-4)

/* ---- ABI structs (layout identical to the reference's) --------------------------------- */

/* engine.h:219-222 */
typedef struct sa_hip_pair_u32 {
    uint32_t first;
    uint32_t second;
} sa_hip_pair_u32;

/* engine.h:123-130 SuffixArray_struct; sizeof == 40.  is_quoted_bitflag is opaque here. */
typedef struct sa_hip_SuffixArray_struct {
    uint32_t* suffix_array;
    void*     is_quoted_bitflag;
    uint64_t  global_byte_start_idx;
    uint64_t  global_byte_end_idx;
    uint32_t  max_suffix_length;
    uint32_t  n;
} sa_hip_SuffixArray_struct;

/* ---- (1) construction, libsais-call-compatible (host pointers in, host SA out) ---------- */

/* replaces libsais (libsais.h:84, libsais.c:6618).  SA[0..n) <- suffix array of T[0..n);
 * SA[n..n+fs) untouched; freq (if non-NULL) <- 256-bin byte histogram. */
int32_t sa_hip_libsais(const uint8_t* T, int32_t* SA, int32_t n, int32_t fs, int32_t* freq);
/* replaces libsais_omp (libsais.h:121, libsais.c:6791).  threads is validated (>= 0) and
 * otherwise ignored: the device pipeline has no host thread pool. */
int32_t sa_hip_libsais_omp(const uint8_t* T, int32_t* SA, int32_t n, int32_t fs, int32_t* freq, int32_t threads);
/* replaces libsais64 (libsais64.h:61, libsais64.c:6657) for n <= UINT32_MAX - 1: 32-bit device
 * build + widening (the reference does the same on the CPU for n <= INT32_MAX, libsais64.c:6670-6682).
 * n > 2^32 - 2 (round 4): the counterpart of the reference's true 64-bit path (libsais64.c:6684 -> libsais64_main) --
 * 64-bit suffix indices on the device (csrc/big_build.hpp: radix sort of (u64 key, u64 suffix) records + prefix doubling
 * on what stays tied), 41 bytes of HBM per character: texts up to about 6.5e9 bytes on one 288 GB GPU, SA_HIP_ENOMEM (-2)
 * beyond.  A functional completion, outside every BASELINE configuration: plain (unpinned) copies, no shared workspace. */
int64_t sa_hip_libsais64(const uint8_t* T, int64_t* SA, int64_t n, int64_t fs, int64_t* freq);
/* replaces libsais64_omp (libsais64.h:86, libsais64.c:6783). */
int64_t sa_hip_libsais64_omp(const uint8_t* T, int64_t* SA, int64_t n, int64_t fs, int64_t* freq, int64_t threads);

/* The 64-bit-index build on device buffers (what sa_hip_libsais64 runs for n > 2^32 - 2; any n >= 0 is accepted, which is how
 * the tests compare it with the oracle at small sizes): text_dev = n bytes, 16-byte aligned; sa_dev = n int64 entries
 * (libsais64 layout).  No index handle is involved: the array is the product. */
typedef struct sa_hip_big_stats {
    uint32_t sigma, bits_per_symbol, initial_chars;   /* alphabet, bits per character code, characters in the initial key  */
    uint32_t sort_passes;                             /* 8-bit radix passes over (u64, u64) records, all sorts of the build */
    uint32_t rounds;                                  /* prefix-doubling rounds                                             */
    uint32_t pad_;
    uint64_t tied_after_sort;                         /* suffixes still tied after the initial sort                         */
    uint64_t tied_total;                              /* sum over the rounds of the tied suffixes they looked at            */
    float    total_ms;                                /* device time of the build (HIP events)                              */
} sa_hip_big_stats;
int sa_hip_libsais64_device(const void* text_dev, int64_t* sa_dev, int64_t n, int device, sa_hip_big_stats* stats /* or NULL */);
/* sufcheck with 64-bit indices: *violations = slots at which sa_dev is not a permutation of [0, n) in suffix order
 * (0 <=> it is THE suffix array of text_dev; 8 n bytes of scratch) */
int sa_hip_sufcheck64_device(const void* text_dev, const int64_t* sa_dev, int64_t n, int device, uint64_t* violations);

/* The four calls above (and sa_hip_construct_truncated_suffix_array) share ONE process-level workspace: a device index
 * whose buffers are allocated on the first call and grow on demand (about 18 bytes of HBM per character of the
 * largest text seen) and 512 MB of pinned host slabs through which the text goes up and the suffix array comes down
 * (as u32 over PCIe, widened to int64 by host threads for the libsais64 forms).  Calls are serialised on it. */
typedef struct sa_hip_call_breakdown {
    uint64_t n;
    uint32_t workspace_reused;   /* 1: no device or pinned allocation in this call                           */
    uint32_t pad_;
    double   total_ms;           /* wall time of the call                                                   */
    double   workspace_ms;       /* creating / growing the workspace                                        */
    double   upload_ms;          /* text: pageable host memory -> pinned slabs -> HBM                        */
    double   build_ms;           /* wall time of the device build incl. its host synchronisations           */
    double   build_device_ms;    /* ... HIP-event time of the same                                          */
    double   download_ms;        /* suffix array: HBM -> pinned slabs -> (widened into) the caller's array  */
} sa_hip_call_breakdown;
/* Where the time of the last of those calls in this process went. */
int sa_hip_last_call_breakdown(sa_hip_call_breakdown* out);
/* Free the shared workspace (device buffers and pinned slabs); the next call allocates it again. */
void sa_hip_release_workspace(void);

/* ---- (1b) LCP arrays, libsais-call-compatible ------------------------------------------------
 * PLCP[i] = length of the longest common prefix of suffix i and the suffix that precedes it in SA order (0 for SA[0]);
 * LCP[r] = PLCP[SA[r]].  Computed on the device by the irreducible-LCP method (csrc/lcp.hpp): only positions whose
 * BWT character differs from their predecessor's are compared against the text, the rest follow from an inclusive
 * max-scan of i + PLCP[i] -- bounded work on highly repetitive texts, where a chunked Kasai pass is quadratic.
 *
 * Drop-ins (host pointers): same arguments, return codes and n <= 1 behaviour as the reference.  threads is validated
 * (>= 0) and otherwise ignored.  LCP may be SA (libsais.h:351).  *_lcp gathers whatever PLCP it is given.  NULL
 * pointers and n < 0 return -1 before any device call; every SA entry is range-checked on the device before it is used,
 * an entry >= n (or < 0) returns -1 and leaves the output undefined.  An in-range SA that is not a suffix array gives
 * unspecified (but bounded) output.  They share the process workspace of sa_hip_libsais* (its pinned slabs; the LCP
 * scratch -- about 16 bytes per character, 32 for the 64-bit forms -- stays allocated until sa_hip_release_workspace)
 * and report in sa_hip_last_call_breakdown (build_ms / build_device_ms = the device pass).  The 64-bit forms run with
 * 64-bit indices on the device and accept every n the 64-bit build accepts, including n > 2^32 - 2. */
/* replaces libsais_plcp (libsais.h:333, libsais.c:7869) */
int32_t sa_hip_libsais_plcp(const uint8_t* T, const int32_t* SA, int32_t* PLCP, int32_t n);
/* replaces libsais_plcp_omp (libsais.h:365, libsais.c:7924) */
int32_t sa_hip_libsais_plcp_omp(const uint8_t* T, const int32_t* SA, int32_t* PLCP, int32_t n, int32_t threads);
/* replaces libsais_lcp (libsais.h:353, libsais.c:7905) */
int32_t sa_hip_libsais_lcp(const int32_t* PLCP, const int32_t* SA, int32_t* LCP, int32_t n);
/* replaces libsais_lcp_omp (libsais.h:387, libsais.c:7964) */
int32_t sa_hip_libsais_lcp_omp(const int32_t* PLCP, const int32_t* SA, int32_t* LCP, int32_t n, int32_t threads);
/* replace libsais64_plcp / _omp and libsais64_lcp / _omp (libsais64.h:220-253) */
int64_t sa_hip_libsais64_plcp(const uint8_t* T, const int64_t* SA, int64_t* PLCP, int64_t n);
int64_t sa_hip_libsais64_plcp_omp(const uint8_t* T, const int64_t* SA, int64_t* PLCP, int64_t n, int64_t threads);
int64_t sa_hip_libsais64_lcp(const int64_t* PLCP, const int64_t* SA, int64_t* LCP, int64_t n);
int64_t sa_hip_libsais64_lcp_omp(const int64_t* PLCP, const int64_t* SA, int64_t* LCP, int64_t n, int64_t threads);

/* Where the device time of an LCP call went (HIP events) and how much text it compared. */
typedef struct sa_hip_lcp_stats {
    uint64_t n;
    uint64_t tied;                 /* ranks whose packed key equals the predecessor's (0 when the key shortcut is off)       */
    uint64_t compared_positions;   /* irreducible positions compared against the text                                        */
    uint64_t compared_bytes;       /* text bytes compared (pairs of bytes, counted once)                                      */
    uint64_t wave_compares;        /* pairs longer than the per-lane budget, compared by one wave each                         */
    uint64_t split_compares;       /* pairs longer than the per-wave budget, compared across workgroups                        */
    uint32_t split_rounds;         /* rounds of doubling segments launched for them                                           */
    uint32_t keys;                 /* 1: the key shortcut of an index handle was used                                         */
    double   phi_ms;               /* range check, reducibility test, short comparisons, scatter                              */
    double   wave_ms;
    double   split_ms;
    double   scan_ms;              /* max-scan of i + PLCP[i] over the text                                                   */
    double   gather_ms;            /* LCP[r] = PLCP[SA[r]] (0 for a PLCP output)                                              */
    double   total_ms;
} sa_hip_lcp_stats;

/* The 64-bit forms on device buffers (mirror sa_hip_libsais64_device; any n >= 0): text_dev n bytes, 8-byte aligned;
 * sa_dev n int64 entries; out_dev n int64 entries (PLCP in text order, or LCP in SA order).  Synchronous; stats may be
 * NULL.  An SA entry outside [0, n) returns -1. */
int sa_hip_plcp64_device(const void* text_dev, const int64_t* sa_dev, int64_t* out_dev, int64_t n, int device, sa_hip_lcp_stats* stats);
int sa_hip_lcp64_device(const void* text_dev, const int64_t* sa_dev, int64_t* out_dev, int64_t n, int device, sa_hip_lcp_stats* stats);

/* ---- (1c) BWT / inverse BWT, libsais-call-compatible ------------------------------------------
 * BWT with libsais' conventions: the primary index is ISA[0] + 1, U[0] = T[n-1], then T[SA[r]-1] for every rank r with
 * SA[r] != 0 in rank order; the aux form writes I[t] = ISA[t*r] + 1 for t = 0..(n-1)/r (r a power of two >= 2).
 * Forward: the suffix array is built on the device and only U (and I) travel back.  Inverse (csrc/bwt.hpp): psi by a
 * stable counting sort of U, then bounded walks over ruler sets (at most B dependent steps per lane), the rulers ranked
 * by pointer jumping on the device -- libsais_unbwt with r = n is sequential even in its _omp form.
 *
 * Drop-ins (host pointers): same arguments, return codes and n <= 1 behaviour as the reference.  threads is validated
 * (>= 0) and otherwise ignored; A is validated (non-NULL) and not used; U may be T.  NULL pointers, n < 0, fs < 0, an r
 * that is not a power of two >= 2 (unbwt: or n), an aux index outside (0, n], and n <= 1 with I[0] != n return -1 before
 * any device call.  Difference: unbwt never reads freq -- the device computes the histogram of T itself, so a wrong
 * table cannot misplace anything (the reference decodes garbage there).  Input that is not the BWT of any text returns
 * 0 as in the reference, with unspecified (but bounded) output.  -2 means more walk rounds or rulers than the bounds
 * allow (not expected).  They share the process workspace of sa_hip_libsais* and report in sa_hip_last_call_breakdown.
 * The 64-bit forms take every n the 64-bit build takes, including n > 2^32 - 2 (64-bit indices on the device there). */
/* replaces libsais_bwt (libsais.h:147, libsais.c:6665) */
int32_t sa_hip_libsais_bwt(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq);
/* replaces libsais_bwt_omp (libsais.h:203) */
int32_t sa_hip_libsais_bwt_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq, int32_t threads);
/* replaces libsais_bwt_aux (libsais.h:161, libsais.c:6691) */
int32_t sa_hip_libsais_bwt_aux(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq, int32_t r, int32_t* I);
/* replaces libsais_bwt_aux_omp (libsais.h:218) */
int32_t sa_hip_libsais_bwt_aux_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, int32_t fs, int32_t* freq, int32_t r, int32_t* I, int32_t threads);
/* replaces libsais_unbwt (libsais.h:254, libsais.c:7588) */
int32_t sa_hip_libsais_unbwt(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t i);
/* replaces libsais_unbwt_omp (libsais.h:308) */
int32_t sa_hip_libsais_unbwt_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t i, int32_t threads);
/* replaces libsais_unbwt_aux (libsais.h:280, libsais.c:7598-7614) */
int32_t sa_hip_libsais_unbwt_aux(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t r, const int32_t* I);
/* replaces libsais_unbwt_aux_omp (libsais.h:322) */
int32_t sa_hip_libsais_unbwt_aux_omp(const uint8_t* T, uint8_t* U, int32_t* A, int32_t n, const int32_t* freq, int32_t r, const int32_t* I, int32_t threads);
/* replace libsais64_bwt / _aux / _omp and libsais64_unbwt / _aux / _omp (libsais64.h:112-209) */
int64_t sa_hip_libsais64_bwt(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq);
int64_t sa_hip_libsais64_bwt_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq, int64_t threads);
int64_t sa_hip_libsais64_bwt_aux(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq, int64_t r, int64_t* I);
int64_t sa_hip_libsais64_bwt_aux_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, int64_t fs, int64_t* freq, int64_t r, int64_t* I, int64_t threads);
int64_t sa_hip_libsais64_unbwt(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t i);
int64_t sa_hip_libsais64_unbwt_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t i, int64_t threads);
int64_t sa_hip_libsais64_unbwt_aux(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t r, const int64_t* I);
int64_t sa_hip_libsais64_unbwt_aux_omp(const uint8_t* T, uint8_t* U, int64_t* A, int64_t n, const int64_t* freq, int64_t r, const int64_t* I, int64_t threads);

/* Where the device time of a BWT or inverse BWT call went (HIP events) and how its walks ran. */
typedef struct sa_hip_bwt_stats {
    uint64_t n;
    uint64_t rulers;               /* inverse: rulers walked (aux rows, hash-chosen rows, rows claimed by long walks)         */
    uint64_t longest_walk;         /* inverse: most psi steps one lane ran in one launch (<= the walk bound B)                */
    uint32_t ruler_rounds;         /* inverse: walk launches (1 + rounds started from claimed rulers)                         */
    uint32_t rank_rounds;          /* inverse: pointer-jumping rounds (0 on the aux-only plan)                                */
    uint32_t aux_only;             /* inverse: 1 = aux rows were the rulers, offsets known, no ranking                        */
    uint32_t pad_;
    double   psi_ms;               /* inverse: histogram, scan, psi                                                           */
    double   walk_ms;              /* inverse: ruler placement and walks                                                      */
    double   rank_ms;
    double   copy_ms;              /* inverse: staging slots to the output                                                    */
    double   gather_ms;            /* forward: range check, primary / aux rows, U                                             */
    double   total_ms;
} sa_hip_bwt_stats;

/* On device buffers, 64-bit indices (mirror sa_hip_plcp64_device; any n >= 0; synchronous; stats may be NULL).
 * bwt64: text_dev n bytes, sa_dev n int64 entries, U_dev n bytes (may be text_dev), I_dev NULL or (n-1)/r + 1 int64
 * entries with r a power of two >= 2.  Returns the primary index (I_dev NULL) or 0 (I_dev given), -1 on bad arguments
 * or an SA entry outside [0, n).
 * unbwt64: U_dev n bytes (the BWT), out_dev n bytes (may be U_dev), I_dev (n-1)/r + 1 int64 entries with r == n or a
 * power of two >= 2.  Returns 0, -1 (bad arguments, an I entry outside (0, n]), -2 (not expected). */
int64_t sa_hip_bwt64_device(const void* text_dev, const int64_t* sa_dev, void* U_dev, int64_t n, int64_t r, int64_t* I_dev, int device,
                            sa_hip_bwt_stats* stats);
int sa_hip_unbwt64_device(const void* U_dev, void* out_dev, int64_t n, int64_t r, const int64_t* I_dev, int device, sa_hip_bwt_stats* stats);

/* ---- (1d) integer alphabets, libsais-call-compatible --------------------------------------------
 * Suffix arrays of texts of int32 / int64 symbols in [0, k) (token ids, remapped byte texts, reduced strings), bit for bit
 * the reference's: a suffix that ends sorts before every suffix that continues.  On the device (csrc/int_build.hpp): one
 * alphabet pass (min, max; with max + 1 <= 2^24 a presence table and its scan give dense codes 1 + rank and sigma), then
 *   route A (sigma <= 256, n <= 2^32 - 2): the rank of every symbol as a byte, and the byte build of sa_hip_libsais;
 *   route B (everything else): floor(64 / b) codes of b bits per suffix as the initial key, the radix sort and prefix doubling
 *   of the 64-bit build (sa_hip_libsais64_device), narrowed to int32 for libsais_int.  About 40 bytes of HBM per symbol plus
 *   the text; -2 beyond what the device holds.
 * Cases answered on the host before any HIP call: NULL T or SA, n < 0, fs < 0, threads < 0 -> -1; n == 0 -> 0; n == 1 ->
 * SA[0] = 0 and 0 (T[0] not looked at, libsais.c:6640); k < 1 with n >= 2 -> -1.  T is never written (the reference may
 * modify and restore it); SA[n .. n+fs) is never touched; threads is validated and otherwise ignored.
 * Deliberate deviation: a symbol outside [0, k) (undefined behaviour in the reference) is found by the alphabet pass and
 * returns -1, with sa_hip_last_error() naming the first such position and value; SA[0..n) is then undefined and the next
 * call works normally.  -2: out of device memory; -3: no usable HIP device.  The drop-ins share the process workspace of
 * sa_hip_libsais* (the pinned slabs; route A: the cached index) and report in sa_hip_last_call_breakdown. */
/* replaces libsais_int (libsais.h:96, libsais.c:6634) */
int32_t sa_hip_libsais_int(int32_t* T, int32_t* SA, int32_t n, int32_t k, int32_t fs);
/* replaces libsais_int_omp (libsais.h:134, libsais.c:6809) */
int32_t sa_hip_libsais_int_omp(int32_t* T, int32_t* SA, int32_t n, int32_t k, int32_t fs, int32_t threads);
/* replaces libsais64_long (libsais64.h:73, libsais64.c:6687); any n the device holds, including n > 2^32 - 2 (route B) */
int64_t sa_hip_libsais64_long(int64_t* T, int64_t* SA, int64_t n, int64_t k, int64_t fs);
/* replaces libsais64_long_omp (libsais64.h:99, libsais64.c:6815) */
int64_t sa_hip_libsais64_long_omp(int64_t* T, int64_t* SA, int64_t n, int64_t k, int64_t fs, int64_t threads);
/* replaces libsais_plcp_int (libsais.h:343, libsais.c:7887): PLCP over int32 symbols by the irreducible method of (1b); every
 * SA entry is range-checked on the device, an entry outside [0, n) returns -1.  n == 1 gives PLCP[0] = 0 on the host.
 * sa_hip_libsais_lcp turns its result into LCP unchanged. */
int32_t sa_hip_libsais_plcp_int(const int32_t* T, const int32_t* SA, int32_t* PLCP, int32_t n);
/* replaces libsais_plcp_int_omp (libsais.h:376, libsais.c:7944) */
int32_t sa_hip_libsais_plcp_int_omp(const int32_t* T, const int32_t* SA, int32_t* PLCP, int32_t n, int32_t threads);

/* How an integer build ran (device forms below). */
typedef struct sa_hip_int_stats {
    uint64_t n;
    uint32_t plan;                 /* 0 = byte pipeline (route A), 1 = integer keys (route B)                                 */
    uint32_t sigma;                /* distinct symbols; 0 = not counted (max + 1 > 2^24, or compaction off)                   */
    uint32_t compacted;            /* 1: codes are 1 + the rank of the symbol; 0: raw v + 1                                   */
    uint32_t bits_per_symbol;      /* code width in the initial key                                                           */
    uint32_t symbols_per_key;      /* symbols in the initial key (route B: the first doubling step)                           */
    uint32_t sort_passes;          /* radix passes (route A: onesweep launches; route B: 8-bit passes over (u64, u64) records) */
    uint32_t rounds;               /* refinement (route A) or prefix-doubling (route B) rounds                                */
    uint32_t pad_;
    uint64_t tied_after_sort;      /* route B: suffixes still tied after the initial sort                                     */
    uint64_t tied_total;           /* sum over the rounds of the tied suffixes they looked at                                 */
    int64_t  min_symbol;
    int64_t  max_symbol;
    double   alphabet_ms;          /* device time of the alphabet pass                                                        */
    double   total_ms;             /* device time of the whole call (allocation excluded)                                     */
} sa_hip_int_stats;

/* On device buffers, synchronous, stats may be NULL; same results and error codes as the drop-ins (n == 1 writes SA_dev[0] = 0).
 * T_dev is only read.  libsais64_long_device writes SA_dev as the 64-bit build's sort buffer. */
int sa_hip_libsais_int_device(const int32_t* T_dev, int32_t* SA_dev, int32_t n, int32_t k, int device, sa_hip_int_stats* stats);
int sa_hip_libsais64_long_device(const int64_t* T_dev, int64_t* SA_dev, int64_t n, int64_t k, int device, sa_hip_int_stats* stats);
/* PLCP of an int32 text on device buffers (a T_dev that is not 8-byte aligned, or of odd n, is copied into a padded buffer
 * first); an SA entry outside [0, n) returns -1. */
int sa_hip_plcp_int_device(const int32_t* T_dev, const int32_t* SA_dev, int32_t* PLCP_dev, int32_t n, int device, sa_hip_lcp_stats* stats);
/* sufcheck of an int64 text: *violations = slots at which SA_dev is not a permutation of [0, n) in suffix order (0 <=> it is
 * THE suffix array of T_dev; 8 n bytes of scratch) */
int sa_hip_sufcheck_long_device(const int64_t* T_dev, const int64_t* SA_dev, int64_t n, int device, uint64_t* violations);

/* ---- (2) truncated construction, engine.c-call-compatible ------------------------------- */

/* replaces construct_truncated_suffix_array (engine.h:213, engine.c:837-866).
 * Fills the caller-allocated sa->suffix_array[0..sa->n) with the suffixes of text[0..sa->n)
 * ordered by their first min(sa->max_suffix_length, n) bytes (unsigned, a suffix that ends
 * sorts first), ties in text order.  Returns 0 or a negative SA_HIP_* code (the reference
 * returns void and exit()s on failure). */
int sa_hip_construct_truncated_suffix_array(const char* text, sa_hip_SuffixArray_struct* sa);

/* ---- (3) query -------------------------------------------------------------------------- */

/* replaces get_substring_positions (engine.h:229-233, engine.c:869-918): one query, host
 * text (n bytes; a trailing NUL is not required) and host SA.  COMPATIBILITY SHIM, O(n) PER CALL: it creates a
 * private index, uploads text and SA and rebuilds the key array and the directory for ONE query.  Anything that
 * asks more than once must use the handle API below (sa_hip_index_load once, then sa_hip_query_batch). */
sa_hip_pair_u32 sa_hip_get_substring_positions(const char* str, const sa_hip_SuffixArray_struct* sa,
                                               const char* substring);

/* ---- (4) handle API: text + SA resident in HBM ------------------------------------------ */

typedef struct sa_hip_index sa_hip_index;

/* Number of HIP devices visible to this process, or a negative SA_HIP_* code. */
int sa_hip_device_count(void);

/* Create an empty index bound to `device` with capacity for texts of up to n_max bytes
 * (device workspace is allocated here, not in the build call). n_max <= UINT32_MAX - 1. */
int sa_hip_index_create(sa_hip_index** out, uint64_t n_max, int device);
void sa_hip_index_destroy(sa_hip_index* idx);

/* Build from a host text (H2D copy + device build).  max_suffix_length == 0: full suffix
 * array (libsais order); > 0: truncated order as in (2). */
int sa_hip_index_build(sa_hip_index* idx, const uint8_t* T_host, uint64_t n, uint32_t max_suffix_length);
/* Same, text already in device memory of idx's device (copied device-to-device into the index). */
int sa_hip_index_build_device(sa_hip_index* idx, const void* T_dev, uint64_t n, uint32_t max_suffix_length);
/* Build + libsais64 layout in one call (replaces libsais64 on device buffers, libsais64.c:6657-6685): as
 * sa_hip_index_build_device, and sa64_dev[i] = (int64_t)SA[i] for i in [0, n), sa64_dev a device buffer of n * 8 bytes
 * on the index's device.  The widening is not a pass of its own here: on the narrow-record plan the last pass of the
 * sort stores every suffix index as u32 (the index's own array) and as int64 (sa64_dev), and the few slots refined
 * afterwards are patched; other plans end with the widening kernel.  total_ms of the build statistics covers all of it. */
int sa_hip_index_build_device64(sa_hip_index* idx, const void* T_dev, uint64_t n, uint32_t max_suffix_length, void* sa64_dev);
/* Adopt an existing suffix array (host pointers): uploads T and SA and prepares the query
 * structures; SA must be sorted by the first max_suffix_length bytes (0 = fully sorted).
 * Every entry is range-checked on the device: an array with an entry >= n is refused (-1). */
int sa_hip_index_load(sa_hip_index* idx, const uint8_t* T_host, const uint32_t* SA_host, uint64_t n,
                      uint32_t max_suffix_length);
/* Same with device pointers (multi-GPU replicas: T and SA arrive by RCCL broadcast). */
int sa_hip_index_load_device(sa_hip_index* idx, const void* T_dev, const void* SA_dev, uint64_t n,
                             uint32_t max_suffix_length);

/* Replicas without any rebuilding (no counterpart in the reference).  The query structures of a built
 * index -- text, suffix array, sorted key array, bucket directory -- are plain device buffers; a replica reserves
 * buffers of the same layout, the caller fills them (RCCL broadcast straight into them: sa_hip_comm_replicate_index,
 * or torch.distributed over the same pointers), and commit makes the replica searchable after range-checking the
 * suffix array and the directory's ends on the device.  Nothing is gathered, sorted or searched on the replica. */
typedef struct sa_hip_replica_layout {
    uint64_t n;
    uint32_t max_suffix_length;
    uint32_t key_bytes;          /* 0: no key array (n < 2); 4: u32 narrow keys; 8: u64 keys                */
    uint32_t bits_per_symbol;    /* of the packed keys                                                      */
    uint32_t initial_chars;
    uint32_t dir_bits;
    int32_t  lo_shift;           /* narrow keys: key = (bucket << 56) | (narrow << lo_shift)                */
    uint64_t dir_entries;        /* 2^dir_bits + 1                                                          */
    uint16_t code[256];          /* alphabet compaction of the text                                         */
    uint64_t freq[256];
} sa_hip_replica_layout;
typedef struct sa_hip_replica_buffers {
    void* text; void* sa; void* keys; void* dir;          /* device pointers on the index's device        */
    uint64_t text_bytes, sa_bytes, keys_bytes, dir_bytes;  /* what has to travel                            */
} sa_hip_replica_buffers;
/* Layout and buffers of a built (or loaded) index: the source of a replication. */
int sa_hip_index_replica_layout(sa_hip_index* idx, sa_hip_replica_layout* out);
int sa_hip_index_replica_buffers(sa_hip_index* idx, sa_hip_replica_buffers* out);
/* Destination: allocate buffers for `layout` (n <= the handle's capacity) and return where to receive.  The index has
 * no searchable state until sa_hip_index_replica_commit. */
int sa_hip_index_replica_reserve(sa_hip_index* idx, const sa_hip_replica_layout* layout, sa_hip_replica_buffers* out);
int sa_hip_index_replica_commit(sa_hip_index* idx);

/* Multi-GPU lifecycle without PyTorch (the reference has no distributed code): one process
 * per GPU, RCCL over xGMI, loaded at run time (no link-time dependency; a process that already holds a librccl.so --
 * PyTorch ships one -- gets that copy).  Rank 0 calls sa_hip_comm_unique_id and ships the 128 bytes to the other ranks
 * by whatever it has (MPI, a file, a socket: RCCL's own bootstrap contract); every rank then calls sa_hip_comm_create.
 *   sa_hip_comm_replicate_index  root: a built index; other ranks: an empty handle of sufficient capacity, searchable
 *                                afterwards -- one broadcast per buffer (text, SA, key array, directory) straight into
 *                                reserved buffers, nothing rebuilt (sa_hip_index_replica_*); *bytes_out = bytes moved
 *   sa_hip_comm_allgather_ranges every rank's pairs_per_rank (first, last) pairs -> recv_dev[nranks][pairs_per_rank], on the
 *                                index's own stream (ordered after the search that produced them; asynchronous until
 *                                sa_hip_index_sync)
 * torch.distributed drives the same replica entry points in suffixarray_amd/distributed.py. */
#define SA_HIP_COMM_ID_BYTES 128
typedef struct sa_hip_comm sa_hip_comm;
int sa_hip_comm_unique_id(void* id128);
int sa_hip_comm_create(sa_hip_comm** out, const void* id128, int nranks, int rank, int device);
void sa_hip_comm_destroy(sa_hip_comm* comm);
int sa_hip_comm_rank(const sa_hip_comm* comm);
int sa_hip_comm_size(const sa_hip_comm* comm);
int sa_hip_comm_replicate_index(sa_hip_comm* comm, sa_hip_index* idx, int root, uint64_t* bytes_out);
int sa_hip_comm_allgather_ranges(sa_hip_comm* comm, sa_hip_index* idx, const void* send_dev, uint64_t pairs_per_rank, void* recv_dev);

uint64_t sa_hip_index_n(const sa_hip_index* idx);
uint32_t sa_hip_index_max_suffix_length(const sa_hip_index* idx);
/* Device pointers owned by the index: text (n bytes + zero padding) and SA (uint32[n]). */
const void* sa_hip_index_text_dev(const sa_hip_index* idx);
const void* sa_hip_index_sa_dev(const sa_hip_index* idx);
/* The index's HIP stream (hipStream_t as void*), for event timing by the caller. */
void* sa_hip_index_stream(const sa_hip_index* idx);

/* Copy the suffix array to the host: uint32[n]; int32[n] (libsais layout); int64[n] (libsais64
 * layout, widened on the device). */
int sa_hip_index_get_sa_u32(sa_hip_index* idx, uint32_t* out_host);
int sa_hip_index_get_sa_i64(sa_hip_index* idx, int64_t* out_host);
/* The suffix array in libsais64 layout, device to device: out_dev[i] = (int64_t)SA[i] for i in [0, n), out_dev a
 * device buffer of n * 8 bytes on the index's device (libsais64.c:6248-6259 widens in place on the CPU; this is
 * the same pass as one kernel, 12 bytes of HBM traffic per entry).  Asynchronous on the index's stream; its
 * HIP-event time is reported as sa_hip_build_stats.widen_ms. */
int sa_hip_index_widen_device(sa_hip_index* idx, void* out_dev);
/* PLCP (text order) or LCP (SA order) of a built or loaded index, u32[n] into out_dev, a device buffer of n * 4 bytes on
 * the index's device.  Asynchronous on the index's stream when stats is NULL; with stats the call waits and fills it.
 * The packed keys of the index answer every rank whose first k0 characters differ from its predecessor's without
 * touching the text (the "key shortcut"; tied ranks are compared from depth k0).  Truncated indexes
 * (max_suffix_length > 0) and handles without an index return -1 (sa_hip_last_error says why).  The index's scratch
 * for the pass (about 12 bytes per character) stays with the handle. */
int sa_hip_index_plcp_device(sa_hip_index* idx, void* out_dev, sa_hip_lcp_stats* stats);
int sa_hip_index_lcp_device(sa_hip_index* idx, void* out_dev, sa_hip_lcp_stats* stats);
/* BWT of a built or loaded index into U_dev (n bytes on the index's device), libsais conventions (section 1c).  I_dev
 * NULL: *primary = ISA[0] + 1; else r is a power of two >= 2, I_dev holds (n-1)/r + 1 uint32 entries, I[t] =
 * ISA[t*r] + 1, and *primary = I[0].  Synchronous.  Truncated indexes and handles without an index return -1. */
int sa_hip_index_bwt_device(sa_hip_index* idx, void* U_dev, int64_t r, void* I_dev, int64_t* primary, sa_hip_bwt_stats* stats);
/* 256-bin byte histogram of the indexed text (libsais `freq`). */
int sa_hip_index_get_freq(sa_hip_index* idx, uint64_t* freq256);

/* Batched get_substring_positions (engine.c:869-918 per element).  Pattern i is
 * patterns[offsets[i] .. offsets[i+1]); compare length c = min(len, max_suffix_length) when
 * the index is truncated, len otherwise.  out[i] = {first,last} inclusive SA range;
 * {UINT32_MAX,UINT32_MAX} when every suffix is smaller; miss -> first = lower bound,
 * last = first - 1 (mod 2^32).  An empty pattern matches every suffix: {0, n-1}.
 * Host pointers; H2D/D2H copies are issued on the index's stream. */
int sa_hip_query_batch(sa_hip_index* idx, const uint8_t* patterns, const uint64_t* offsets, uint64_t Q,
                       sa_hip_pair_u32* out);
/* Same with every buffer in device memory (no copies; asynchronous on the index's stream
 * until sa_hip_index_sync).  patterns_dev must stay readable for 8 bytes past offsets[Q]: a pattern's last
 * partial 8-byte word is loaded whole and masked (the host-pointer form pads its staging copy itself). */
int sa_hip_query_batch_device(sa_hip_index* idx, const void* patterns_dev, const void* offsets_dev,
                              uint64_t Q, void* out_dev);
/* The same for Q patterns of ONE length, packed back to back (pattern i = patterns_dev[i * pattern_len ..)): no offsets
 * array -- two 8-byte loads per query less (a batch is bound by the number of memory requests).  The
 * padding rule of sa_hip_query_batch_device applies (8 readable bytes past the last pattern). */
int sa_hip_query_batch_device_fixed(sa_hip_index* idx, const void* patterns_dev, uint64_t pattern_len, uint64_t Q, void* out_dev);
/* Copy up to `cap` suffix positions SA[first .. first+count) to the host (hit materialisation). */
int sa_hip_index_get_sa_range(sa_hip_index* idx, uint64_t first, uint64_t count, uint32_t* out_host);
/* ONE query with its first hits, the latency path of record retrieval (get_matching_records, engine.c:1167-1215,
 * called per query by pyx:209-267): *range as in sa_hip_query_batch, hits[0 .. *nhits) = SA[first .. first + *nhits),
 * *nhits = min(number of hits, max_hits, 4096).  Pattern, range and hits travel through one pinned host block that
 * the kernels read and write directly: two small launches and one synchronisation, no copy calls. */
int sa_hip_index_query_hits(sa_hip_index* idx, const uint8_t* pattern, uint64_t len, uint32_t max_hits,
                            sa_hip_pair_u32* range, uint32_t* hits, uint32_t* nhits);

/* Second-level keys (round 4; csrc/sa_query.hpp): for the SA slots that share their key (first k0 characters) with a neighbour,
 * the next floor(64 / b) characters, packed like the key -- 8 n bytes, one gather over those slots.  A pattern longer than the
 * key then finds its bounds inside a key group by a binary search over 8-byte keys instead of text comparisons (two dependent
 * random reads per step).  Wide-key indexes only (word / name / DNA text; near-random text has no such groups).
 *   mode 1 (the default of every handle): the first batch of >= 32768 patterns builds them on its way;
 *   mode 2: build them now;   mode 0: drop them and never build them (the text search stays).
 * Returns 1 when the index has them afterwards, 0 when not (narrow keys, no memory, mode 0), < 0 on errors.  The results of
 * every query are the same with or without; a rebuild / load / replica commit drops them. */
int sa_hip_index_deep_keys(sa_hip_index* idx, int mode);
int sa_hip_index_sync(sa_hip_index* idx);

/* On-device check that the index's SA is the suffix array of its text (truncated indexes: that
 * it is a permutation ordered by the first max_suffix_length bytes, ties in text order).
 * *violations = 0 means verified.  O(n) device work, 4n bytes of device scratch; the O(n)
 * "sufcheck" that makes bit-exactness testable at n = 1e9 without a CPU oracle run. */
int sa_hip_index_verify(sa_hip_index* idx, uint64_t* violations);

/* ---- (5) record retrieval: hits -> rows (engine.c:920-999, 1168-1215, 1326-1390; bound at pyx:87-101) -------------- */

/* Row table of the indexed text: row r (a document, or one CSV field) = text[row_text_starts[r], row_text_starts[r+1]);
 * row_text_starts[0] must be 0 and the offsets ascend.  The table is copied (under the handle's lock, like every
 * reader of it). */
int sa_hip_index_set_rows(sa_hip_index* idx, const uint64_t* row_text_starts, uint64_t num_rows);
/* ONE query -> the distinct rows that contain the pattern, in SA order of their first hit, at most k of them
 * (row_ids[0 .. *num_rows)); *range (may be NULL) as in sa_hip_query_batch.  The reference returns one record per HIT
 * (engine.c:1364-1388); one per ROW is this library's decision. */
int sa_hip_index_query_rows(sa_hip_index* idx, const uint8_t* pattern, uint64_t len, uint32_t k, uint64_t* row_ids,
                            uint32_t* num_rows, sa_hip_pair_u32* range);
/* The batched form (new surface; per element it is sa_hip_index_query_rows): pattern i = patterns[offsets[i] ..
 * offsets[i+1]); row_ids[i * k .. i * k + counts[i]) = its distinct rows, ranges[i] (may be NULL) its SA range.  ONE search
 * launch finds every range and ONE more launch maps every hit of every range to its row (binary search over the row
 * table in HBM) and de-duplicates per query in LDS (k <= 4096; larger k is served per query on the host): no per-query
 * synchronisation, one copy back.  Replaces the per-query loop of suffix_array.pyx:221-247 over engine.c:1364-1388.
 * In a batch of 4096 queries or more, ranges of at most 4 hits are answered by one lane each, longer ones by one wave each
 * (k <= 64) or one workgroup each; when Q * k row ids exceed 32 MiB the host legs go through the process's ring of pinned slabs (512 MiB, shared with
 * the sa_hip_libsais* wrappers, given back by sa_hip_release_workspace) and the ids are widened into row_ids by worker threads.
 * row_ids, counts and ranges are the caller's arrays (entries of row_ids beyond counts[i] are left untouched): keep them from
 * call to call. */
int sa_hip_index_query_rows_batch(sa_hip_index* idx, const uint8_t* patterns, const uint64_t* offsets, uint64_t Q, uint32_t k,
                                  uint64_t* row_ids, uint32_t* counts, sa_hip_pair_u32* ranges);
/* The same for a range that a batched query has already found (sa_hip_query_batch: one launch for all the ranges,
 * then the rows per range). */
int sa_hip_index_rows_for_range(sa_hip_index* idx, sa_hip_pair_u32 range, uint32_t k, uint64_t* row_ids, uint32_t* num_rows);
/* Copy the indexed text (n bytes) back to the host (persistence: the CSV-mode text is the extracted column). */
int sa_hip_index_get_text(sa_hip_index* idx, uint8_t* out_host);

/* CSV-mode index: replaces SuffixArrayIndex + construct_truncated_suffix_array_from_csv_partitioned_mmap_full
 * (engine.h:163-172, engine.c:1454-1482 -> 461-654): extracts `search_column` of an RFC-4180 file (lower-cased, one
 * '\n' after every field, header row not indexed, 64-bit file offsets), builds the device index over it with
 * max_suffix_length and keeps the row tables + a read-only mapping of the file.  One index per file: the 2 GiB
 * partitioning of the reference (engine.c:1437) is not reproduced (288 GB of HBM; the column must stay below 2^32 - 2
 * bytes). */
typedef struct sa_hip_csv_index sa_hip_csv_index;
int sa_hip_csv_index_create(sa_hip_csv_index** out, const char* csv_file, const char* search_column, uint32_t max_suffix_length,
                            int device);
/* Re-open a saved CSV-mode index without parsing or building (persistence; the reference's
 * read_suffix_array is declared but never defined, engine.h:141): adopts text + SA + row tables; column_names =
 * num_columns NUL-terminated names back to back. */
int sa_hip_csv_index_adopt(sa_hip_csv_index** out, const char* csv_file, const uint8_t* text, const uint32_t* SA, uint64_t n,
                           const uint64_t* row_text_starts, const uint64_t* row_file_offsets, uint64_t num_rows,
                           const char* column_names, uint32_t num_columns, uint32_t column_index, uint32_t max_suffix_length,
                           int device);
void sa_hip_csv_index_destroy(sa_hip_csv_index* c);
/* The same rows without the copies: row_ptrs[i] points INTO the index's read-only mapping of the CSV file (row_lens[i] bytes, line
 * terminator excluded, NOT NUL-terminated), valid until the index is destroyed; at most k rows, *num_matches = how many.  New
 * surface (the reference's interface mallocs every record, engine.c:1382): what a binding uses when it builds its own objects
 * from the bytes anyway. */
int sa_hip_get_matching_row_spans_file(sa_hip_csv_index* c, const char* substring, uint32_t k, const char** row_ptrs,
                                       uint32_t* row_lens, uint32_t* num_matches);
/* A column of more than `partition_bytes` (0 or > 2^32 - 2: 2^32 - 2) bytes as several independent indexes of WHOLE rows over
 * the same file: the reference's partitions (engine.c:1437-1481 cuts the FILE every 2 GiB; suffix_array.pyx:221-247 answers
 * from the partitions one after the other).  *out_parts: malloc'ed array of *num_parts handles (>= 1; each is destroyed with
 * sa_hip_csv_index_destroy, the array with sa_hip_csv_index_free_parts); every sa_hip_csv_index entry point works on a part.
 * The file is parsed once. */
int sa_hip_csv_index_create_partitioned(sa_hip_csv_index*** out_parts, uint32_t* num_parts, const char* csv_file, const char* search_column,
                                        uint32_t max_suffix_length, int device, uint64_t partition_bytes);
void sa_hip_csv_index_free_parts(sa_hip_csv_index** parts);
/* The device index underneath (batched queries, statistics, verification); owned by the CSV index. */
sa_hip_index* sa_hip_csv_index_handle(sa_hip_csv_index* c);
uint64_t sa_hip_csv_index_num_rows(const sa_hip_csv_index* c);
uint32_t sa_hip_csv_index_num_columns(const sa_hip_csv_index* c);
uint32_t sa_hip_csv_index_column_index(const sa_hip_csv_index* c);
const char* sa_hip_csv_index_column_name(const sa_hip_csv_index* c, uint32_t i);
/* Borrowed views of the row tables: row_text_starts[num_rows], row_file_offsets[num_rows + 1]. */
int sa_hip_csv_index_row_tables(const sa_hip_csv_index* c, const uint64_t** row_text_starts, const uint64_t** row_file_offsets);

/* Rows of the file by id, as malloc'ed NUL-terminated strings without the line terminator (records[0 .. n); ownership
 * as in sa_hip_get_matching_records_file). */
int sa_hip_csv_index_copy_rows(sa_hip_csv_index* c, const uint64_t* row_ids, uint32_t n, char** records);

/* replaces get_substring_positions_file (engine.h:235-239, engine.c:920-999): the search of CSV mode.  The reference
 * reads the text per probe from the file (fseek + fread + tolower); here it is the batched kernel with Q = 1 over the
 * extracted column in HBM.  Result conventions of THAT function: a hit -> inclusive range {first, last} over the
 * index's suffix array; ANY miss -> {UINT32_MAX, UINT32_MAX} (engine.c:962-965).  `substring` is compared as given
 * (the reference's caller lower-cases it, pyx:228). */
sa_hip_pair_u32 sa_hip_get_substring_positions_file(sa_hip_csv_index* c, const char* substring);
/* replaces get_matching_records_file (engine.h:257-264, engine.c:1326-1390; bound at pyx:94-101, called at pyx:224-232):
 * appends the rows that contain `substring` to matching_records[*num_matches ...] until *num_matches == k.  Ownership
 * as in the reference: every row is a malloc'ed NUL-terminated string (engine.c:1382), the caller frees each one
 * (pyx:262-265; or sa_hip_free_records).  Differences by decision: a row is returned once however
 * often it contains the pattern, rows come back whole (engine.c:1314 drops the last character), a miss appends
 * nothing.  Returns 0 or a negative SA_HIP_* code (the reference returns void and exit()s). */
int sa_hip_get_matching_records_file(sa_hip_csv_index* c, const char* substring, uint32_t k, char** matching_records,
                                     uint32_t* num_matches);
/* replaces get_matching_records (engine.h:249-255, engine.c:1168-1215; bound at pyx:87-93): host text + host SA, the
 * records are the lines of `str` ('\n'-separated documents) that contain the pattern; returns their number (<= k).
 * Like sa_hip_get_substring_positions this uploads text and SA for ONE query -- O(n) per call: a compatibility shim,
 * not the fast path (use a handle + sa_hip_index_set_rows + sa_hip_index_query_rows). */
uint32_t sa_hip_get_matching_records(const char* str, const sa_hip_SuffixArray_struct* sa, const char* substring, uint32_t k,
                                     char** matching_records);
/* free() every row of a result table (the table itself belongs to the caller). */
void sa_hip_free_records(char** records, uint32_t n);

/* replaces init_suffix_array_byte_idxs / free_suffix_array (engine.h:133-140, engine.c:326-349; pyx:68-74): malloc /
 * free of the caller-side uint32 suffix_array[n] of a SuffixArray_struct for the engine-compatible calls of (2) and
 * (3).  is_quoted_bitflag is left NULL: the row tables of sa_hip_csv_index replace the reference's per-character
 * quoted bits (engine.c:637-645), which only serve its newline seeks. */
int sa_hip_init_suffix_array_byte_idxs(sa_hip_SuffixArray_struct* sa, uint32_t max_suffix_length, uint64_t global_byte_start_idx,
                                       uint64_t global_byte_end_idx, uint32_t n);
void sa_hip_free_suffix_array(sa_hip_SuffixArray_struct* sa);

/* replaces write_suffix_array (engine.h:142-146, engine.c:1112-1138) and read_suffix_array (declared at engine.h:141, never
 * defined in the reference): the reference's own file layout {u64 global_byte_start_idx, u64 global_byte_end_idx,
 * u32 max_suffix_length, u32 n, u32 suffix_array[n]}, so that an index file of either side can be read by the other.
 * is_quoted_filename (may be NULL) receives an empty bit buffer {u32 capacity = 0} (engine.c:1098-1101): this library
 * keeps row tables instead of per-character quoted bits.  The reader mallocs suffix_array (sa_hip_free_suffix_array) and
 * refuses entries >= n.  Note for CSV mode: the reference stores FILE byte offsets in the array (engine.c:648-651), this
 * library positions of the extracted column; SuffixArray.save / load of the Python class keep the row tables beside it. */
int sa_hip_write_suffix_array(const sa_hip_SuffixArray_struct* sa, const char* sa_filename, const char* is_quoted_filename);
int sa_hip_read_suffix_array(sa_hip_SuffixArray_struct* sa, const char* sa_filename);

/* ---- (6) token index: n-gram ranges, longest-suffix spans and next-symbol counts over an int32 text and its suffix array ----
 * The search side of section (1d) (no counterpart in the reference): the text (int32 symbols in [0, 2^31 - 1]) and its suffix
 * array (int32, what sa_hip_libsais_int[_device] produces; n <= 2^31 - 1) stay in HBM with two search structures -- a
 * first-symbol directory (when max - min + 1 <= 2^24) and an array of 8-byte keys over the first two symbols of every suffix in
 * suffix order (csrc/token_query.hpp).  4 + 4 + 8 bytes per symbol plus the directory.  A handle of its own: sa_hip_index and
 * the byte query of section (4) are not involved.
 *
 * Results are {first, second} = {number of suffixes that sort before the pattern (a suffix that ends sorts before one that
 * continues), number of suffixes that have the pattern as a prefix}: its occurrences are SA[first .. first + second).  A miss
 * has second == 0 and first is still the exact lower bound; an empty pattern gives {0, n}.  There is no UINT32_MAX and no
 * "last = first - 1" form here.  Pattern symbols may be any int32 (a negative one sorts below every text symbol), patterns any
 * length, also longer than the text; Q == 0 is a no-op.
 *
 * Errors: NULL pointers, n < 0 and k < 1 with n >= 2 return -1 before any HIP call (T may be NULL when n == 0; n == 0 and
 * n == 1 give a handle that answers queries); no usable device -3 (never a fallback); out of device memory -2; a negative text
 * symbol, or (load) an SA entry outside [0, n): -1.  An in-range array that is not the suffix array gives unspecified results
 * from bounded loops (a search is at most 32 steps, a comparison at most the pattern's length).  A handle owns a non-blocking
 * stream and a mutex; the device form of the query is asynchronous until sa_hip_token_index_sync, the host form stages
 * through buffers of the handle.  Nothing is read beyond offsets[Q] symbols of the patterns. */
typedef struct sa_hip_token_index sa_hip_token_index;

typedef struct sa_hip_token_info {
    uint64_t n;
    int64_t  min_symbol;         /* of the text (0 when n == 0)                                                      */
    int64_t  max_symbol;
    uint64_t dir_entries;        /* max - min + 2; 0: no directory (range beyond 2^24, n == 0, or switched off)      */
    uint32_t key_bytes;          /* 8: the key array exists; 0: it does not (n == 0, or switched off)                */
    uint32_t last_rank;          /* the rank of suffix n - 1                                                         */
    double   prepare_ms;         /* device time of the search structures (alphabet, range check, directory, keys)    */
    uint64_t q;                  /* patterns of the last search launch                                               */
    double   kernel_ms;          /* HIP-event time of the last search launch (the call waits for it)                 */
} sa_hip_token_info;

/* Host text: upload, suffix array by the integer build of (1d) (same routes, same errors as sa_hip_libsais_int: symbols in
 * [0, k); k == INT32_MAX admits 2^31 - 1 as a symbol as well), search structures. */
int sa_hip_token_index_build(sa_hip_token_index** out, const int32_t* T_host, int32_t n, int32_t k, int device);
/* Adopt a text and its suffix array that are already on `device` (both copied into the handle). */
int sa_hip_token_index_load_device(sa_hip_token_index** out, const int32_t* T_dev, const int32_t* SA_dev, int32_t n, int device);
void sa_hip_token_index_destroy(sa_hip_token_index* t);
/* Pattern i = patterns[offsets[i] .. offsets[i+1]) (offsets in symbols, Q + 1 of them); out[i] as above.  Host pointers. */
int sa_hip_token_index_query_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, sa_hip_pair_u32* out);
/* Every buffer in device memory; no copies, asynchronous on the handle's stream. */
int sa_hip_token_index_query_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q, void* out_dev);
int sa_hip_token_index_sync(sa_hip_token_index* t);
/* Device pointers owned by the handle: text (int32[n]) and suffix array (int32[n]). */
const void* sa_hip_token_index_text_dev(const sa_hip_token_index* t);
const void* sa_hip_token_index_sa_dev(const sa_hip_token_index* t);
/* Copy SA[first .. first + count) to the host (the positions of a range); first + count > n returns -1. */
int sa_hip_token_index_get_sa_range(sa_hip_token_index* t, uint64_t first, uint64_t count, int32_t* out_host);
/* Copy entries [first, first + count) of the first-symbol directory (uint32, dir_entries of them: entry j = number of suffixes
 * whose first symbol is < min_symbol + j) or of the key array (uint64, n of them: entry r = ((T[p] + 1) << 32) | (p + 1 < n ?
 * T[p + 1] + 1 : 0), p = SA[r]) to the host, synchronising on the handle's stream.  -1 with a message: the handle has no such
 * structure (dir_entries == 0 / key_bytes == 0 in sa_hip_token_info), first + count lies beyond it, or a NULL pointer. */
int sa_hip_token_index_get_dir_range(sa_hip_token_index* t, uint64_t first, uint64_t count, uint32_t* out_host);
int sa_hip_token_index_get_key_range(sa_hip_token_index* t, uint64_t first, uint64_t count, uint64_t* out_host);
int sa_hip_token_index_info(const sa_hip_token_index* t, sa_hip_token_info* out);

/* (6b) longest-suffix spans and next-symbol counts (csrc/token_next.hpp): given a context, the longest suffix of it that the text
 * holds, and which symbols follow it how often.  All results are exact.
 *
 * A span is the range of a matched prefix: SA[first .. first + count) all start with the same `length` symbols.  Within a span
 * the next symbol T[SA[r] + length] is non-decreasing in r, and the one suffix that ends behind the match (ended) stands first.
 *   mode 0, exact: the span of the whole context, length = its length; a miss keeps the exact lower bound in first, count = 0.
 *   mode 1, longest suffix: the largest L <= min(context length, max_length) (max_length == 0: no cap) such that the last L
 *     symbols of the context have an effective count >= 1 -- count - ended with need_next = 1, count with need_next = 0.
 *     L = 0 gives {0, n, 0, 0}; with n == 0 every span is {0, 0, 0, 0}.
 * The next symbols of a span are the distinct values of T[SA[r] + length] over its suffixes that have one, ascending, each with
 * its multiplicity; at most cap (>= 1) entries per span are written, the cap smallest, to symbols[i * cap ..] and
 * counts[i * cap ..].  Slots beyond heads[i].written are not written.  The answer is complete iff covered == total.
 *
 * Errors: a NULL handle or argument, mode or need_next other than 0 / 1, cap == 0, Q * cap >= 2^31 and descending offsets return
 * -1 before any HIP call; Q == 0 is a no-op.  The device forms are asynchronous on the handle's stream until
 * sa_hip_token_index_sync and chain without a host trip (the span output of one is the span input of the other);
 * sa_hip_token_index_next_batch_device trusts nothing: first and count are clamped to the array, and an array that is not the
 * suffix array gives unspecified entries from bounded loops.  The host forms stage through buffers of the handle. */
typedef struct sa_hip_token_span {
    uint32_t first;    /* as in sa_hip_pair_u32.first                                          */
    uint32_t count;    /* suffixes that have the matched symbols as a prefix                   */
    uint32_t length;   /* matched symbols: SA[first..first+count) all share this prefix        */
    uint32_t ended;    /* 1: SA[first] + length == n (that suffix has no next symbol); else 0  */
} sa_hip_token_span;

typedef struct sa_hip_token_next {
    uint32_t written;   /* entries written for this span, <= cap                               */
    uint32_t covered;   /* sum of the written counts                                           */
    uint32_t total;     /* count - ended: suffixes of the span that have a next symbol         */
    uint32_t reserved;  /* 0                                                                   */
} sa_hip_token_next;

typedef struct sa_hip_token_next_info {
    uint64_t q;            /* contexts or spans of the last launch of either kind               */
    double   spans_ms;     /* HIP-event time of the last span launch (the call waits for it)    */
    double   next_ms;      /* ... of the last next-symbol launch                                */
    uint64_t lane_spans;   /* spans of that launch answered by one lane each (count <= 4)       */
    uint64_t wave_spans;   /* ... walked by one wave each                                       */
} sa_hip_token_next_info;

/* Context i = patterns[offsets[i] .. offsets[i+1]); spans[Q] out.  Host pointers. */
int sa_hip_token_index_spans_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                   int mode, uint32_t max_length, int need_next, sa_hip_token_span* spans);
/* Every buffer in device memory; no copies, asynchronous on the handle's stream. */
int sa_hip_token_index_spans_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                          int mode, uint32_t max_length, int need_next, void* spans_dev);
/* spans_dev: sa_hip_token_span[Q]; symbols_dev: int32[Q * cap]; counts_dev: uint32[Q * cap]; heads_dev: sa_hip_token_next[Q]. */
int sa_hip_token_index_next_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap,
                                         void* symbols_dev, void* counts_dev, void* heads_dev);
/* Both steps from host contexts: spans (may be NULL), symbols, counts and heads out. */
int sa_hip_token_index_next_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                  int mode, uint32_t max_length, int need_next, uint32_t cap,
                                  sa_hip_token_span* spans, int32_t* symbols, uint32_t* counts, sa_hip_token_next* heads);
/* Host spans in (from an earlier call); first + count > n returns -1. */
int sa_hip_token_index_next_of_spans(sa_hip_token_index* t, const sa_hip_token_span* spans, uint64_t Q, uint32_t cap,
                                     int32_t* symbols, uint32_t* counts, sa_hip_token_next* heads);
int sa_hip_token_index_next_info(const sa_hip_token_index* t, sa_hip_token_next_info* out);

/* (6c) shard sets (csrc/token_shards.hpp, csrc/capi_token_shards.hpp): S token indexes on ONE device, 1 <= S <= 64, answered as
 * one corpus that was cut at document boundaries -- an n-gram never spans two shards.  Counts are summed over the shards as
 * uint64, the longest suffix is the longest one that ANY shard holds, next-symbol lists are merged.  Every per-shard array is
 * shard-major: entry [s * Q + i] belongs to shard s and pattern / context i.
 *
 *   ranges  per_shard[s * Q + i] is what shard s's own sa_hip_token_index_query_batch answers for pattern i (a miss keeps the
 *           exact lower bound in first); totals[i] = sum over s of second.  per_shard may be NULL.
 *   spans   mode 0: spans[s * Q + i] is shard s's mode-0 span of the whole context; length[i] = the context's length.
 *           mode 1: L_i = the largest L <= min(context length, max_length) (max_length == 0: no cap) such that the SUM over the
 *           shards of the effective counts of the last L symbols is >= 1 (effective: count - ended with need_next = 1, count
 *           with need_next = 0); spans[s * Q + i] is what shard s's own spans_batch answers in mode 0 for those last L_i symbols:
 *           count 0 with the exact lower bound where the shard does not hold them, {first, 1, L_i, 1} where they only end the
 *           shard's text.  length[i] = L_i.  In both modes totals[i] = the sum of the effective counts.
 *   next    the distinct next symbols over the union of the S spans of a context, ascending, their counts summed as uint64; at
 *           most cap entries, the cap smallest, to symbols[i * cap ..] and counts[i * cap ..]; slots beyond heads[i].written are
 *           not written.  Merging the shards' own cap-smallest lists is exact: a symbol among the union's cap smallest has at
 *           most that rank among the symbols of every shard that holds it.  total = sum over s of (count_s - ended_s), covered =
 *           the sum of the written counts; the answer is complete iff covered == total.  length = the largest `length` among
 *           the context's S spans (0 from sa_hip_token_shards_merge_device, which sees no spans).
 *
 * sa_hip_token_shards_create adopts the handles: the set owns them from then on and sa_hip_token_shards_destroy destroys them;
 * on any error none is adopted.  NULL arguments, S == 0, S > 64, a NULL entry, a repeated entry and handles on different devices
 * return -1 before any HIP call.  The other argument errors are those of (6b): NULL pointers, mode or need_next other than 0 / 1,
 * cap == 0, Q * cap >= 2^31 and descending offsets return -1 before any HIP call; Q == 0 is a no-op; no usable device -3.  A set
 * owns a non-blocking stream and a mutex; the device forms are asynchronous on that stream until sa_hip_token_shards_sync and
 * chain without a host trip.  The per-shard lists of the next-symbol calls live in scratch of the set, S * cap * 8 bytes per
 * context: the batch is worked through in chunks of contexts sized by a scratch budget (sa_hip_token_shards_stats.chunk: the
 * contexts per chunk of the last such call).
 *
 * Matching statistics of a query text over the set -- sa_hip_token_shards_match_* -- stand behind (6f), whose terms and head
 * record they use: see "(6c, matching statistics)" there.  Documents over a set -- locate, the distinct documents of an n-gram and
 * its document frequency, sa_hip_token_shards_locate_* and _docs_* -- are (6g).  Per-document counts and AND groups over a set --
 * sa_hip_token_shards_doc_counts_* and _all_* -- are (6h).  Infinity-gram scores of a query text over a set --
 * sa_hip_token_shards_score_* -- are (6j), behind (6i) whose terms and head record they use. */
typedef struct sa_hip_token_shards sa_hip_token_shards;

typedef struct sa_hip_token_shards_next {
    uint32_t written;   /* entries written for this context, <= cap                            */
    uint32_t length;    /* matched symbols (see above)                                         */
    uint64_t covered;   /* sum of the written counts                                           */
    uint64_t total;     /* suffixes of the S spans that have a next symbol                     */
} sa_hip_token_shards_next;

typedef struct sa_hip_token_shards_stats {
    uint32_t shards;       /* S                                                                            */
    uint32_t chunk;        /* contexts per chunk of the last next-symbol call (0: none yet)                */
    uint64_t tokens;       /* sum of the shards' lengths                                                   */
    uint64_t q;            /* patterns / contexts of the last ranges, spans or next-symbol launch          */
    double   ranges_ms;    /* HIP-event time of the last ranges launch (the call waits for it)             */
    double   spans_ms;     /* ... of the last spans launch                                                 */
    double   next_ms;      /* ... of the per-shard next-symbol launches of the last call, over its chunks  */
    double   merge_ms;     /* ... of its merge launches, over its chunks                                   */
} sa_hip_token_shards_stats;

int sa_hip_token_shards_create(sa_hip_token_shards** out, sa_hip_token_index* const* shards, uint32_t S);
void sa_hip_token_shards_destroy(sa_hip_token_shards* set);
/* The borrowed handle of shard s (NULL: no such shard); the caller serialises its use against the set's calls. */
sa_hip_token_index* sa_hip_token_shards_shard(sa_hip_token_shards* set, uint32_t s);
int sa_hip_token_shards_sync(sa_hip_token_shards* set);
int sa_hip_token_shards_info(const sa_hip_token_shards* set, sa_hip_token_shards_stats* out);
/* totals[Q]; per_shard[S * Q] or NULL.  Host pointers. */
int sa_hip_token_shards_query_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    uint64_t* totals, sa_hip_pair_u32* per_shard);
/* Every buffer in device memory (per_shard_dev may be NULL); asynchronous on the set's stream. */
int sa_hip_token_shards_query_batch_device(sa_hip_token_shards* set, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           void* totals_dev, void* per_shard_dev);
/* length[Q], totals[Q], spans[S * Q].  Host pointers. */
int sa_hip_token_shards_spans_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    int mode, uint32_t max_length, int need_next, uint32_t* length, uint64_t* totals,
                                    sa_hip_token_span* spans);
int sa_hip_token_shards_spans_batch_device(sa_hip_token_shards* set, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           int mode, uint32_t max_length, int need_next, void* length_dev, void* totals_dev,
                                           void* spans_dev);
/* Both steps from host contexts: spans[S * Q] (may be NULL), symbols int32[Q * cap], counts uint64[Q * cap], heads[Q] out. */
int sa_hip_token_shards_next_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                   int mode, uint32_t max_length, int need_next, uint32_t cap, sa_hip_token_span* spans,
                                   int32_t* symbols, uint64_t* counts, sa_hip_token_shards_next* heads);
/* spans_dev: sa_hip_token_span[S * Q] as sa_hip_token_shards_spans_batch_device wrote them; the outputs as above, on the device.
 * Trusts nothing, like sa_hip_token_index_next_batch_device. */
int sa_hip_token_shards_next_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t Q, uint32_t cap,
                                          void* symbols_dev, void* counts_dev, void* heads_dev);
/* The last step of the two calls above on its own: S lists per context as the shards' next-symbol launches write them --
 * symbols_dev int32[S * Q * cap] (row (s * Q + i) * cap, ascending), counts_dev uint32[S * Q * cap], heads_dev
 * sa_hip_token_next[S * Q] (written is clamped to cap) -- merged into out_symbols_dev int32[Q * cap], out_counts_dev
 * uint64[Q * cap], out_heads_dev sa_hip_token_shards_next[Q].  Asynchronous on the set's stream. */
int sa_hip_token_shards_merge_device(sa_hip_token_shards* set, const void* symbols_dev, const void* counts_dev, const void* heads_dev,
                                     uint64_t Q, uint32_t cap, void* out_symbols_dev, void* out_counts_dev, void* out_heads_dev);

/* (6d) documents (csrc/token_docs.hpp, csrc/capi_token_docs.hpp): which documents hold an n-gram, where in them, and in how many
 * documents it occurs (its document frequency).  All results are exact.
 *
 * A handle gets its documents from a table doc_starts[0 .. D) of text positions: document d is T[starts[d] .. starts[d + 1]) with
 * starts[D] = n implied.  Required: D >= 1, starts[0] == 0, non-decreasing, every entry <= n (with n == 0 every entry is 0).  Equal
 * neighbours are empty documents, and those are allowed; doc(p) is the LARGEST d with starts[d] <= p, so an empty document never
 * owns a token.  An occurrence belongs to the document of its FIRST token.  Occurrences that run over a boundary are not filtered:
 * callers separate documents with a token of their own, as the shard sets of (6c) already assume.  A second call replaces the
 * first; D == 0 with a NULL pointer removes the documents.  The handle grows by 8 bytes per token plus 4 (D + 1): a document array
 * DA[r] = doc(SA[r]) and a previous-rank array PV[r] = the largest r' < r with DA[r'] == DA[r] (-1: none), both int32[n].  Within a
 * rank range [a, b), rank r is the first occurrence of its document iff PV[r] < a, which is what the counts below stream.
 *
 *   locate  the occurrences SA[first .. first + min(count, cap)) of a span as (document, offset inside it), in suffix order, to
 *           docs[i * cap ..] and offsets[i * cap ..]; the head is {written = min(count, cap), count}.
 *   docs    examined = budget ? min(count, budget) : count ranks of the span are walked from `first`; distinct = the number of
 *           distinct documents among them; the first min(distinct, cap) of them are written in order of first appearance by rank,
 *           docs[i * cap + j] the document and offsets[i * cap + j] the offset inside it of its smallest-rank occurrence.  The
 *           head is {written, examined, distinct, count}: distinct is the n-gram's exact document frequency iff examined == count.
 *           cap == 0 means counts only; docs and offsets may then be NULL and are never touched.
 * Slots beyond `written` are not written.
 *
 * Errors returned as -1 before any HIP call: a NULL handle or a NULL required pointer, a bad table (set_documents), a handle
 * without documents, mode or need_next other than 0 / 1, cap == 0 in locate, Q * cap >= 2^31 and descending offsets; Q == 0 is a
 * no-op returning 0.  The device forms take sa_hip_token_span[Q] exactly as sa_hip_token_index_spans_batch_device writes them, chain
 * with it without a host trip and are asynchronous until sa_hip_token_index_sync; they trust nothing: first and count are clamped
 * to the array, and an array that is not the suffix array gives unspecified entries from bounded loops.  The host forms run the
 * span step first (locate always in mode 0) and stage through buffers of the handle. */
typedef struct sa_hip_token_locate {
    uint32_t written;    /* entries written for this span: min(count, cap)                      */
    uint32_t count;      /* suffixes of the span                                                */
} sa_hip_token_locate;

typedef struct sa_hip_token_docs {
    uint32_t written;    /* entries written for this span: min(distinct, cap)                   */
    uint32_t examined;   /* ranks walked: budget ? min(count, budget) : count                   */
    uint32_t distinct;   /* distinct documents among the examined ranks                         */
    uint32_t count;      /* suffixes of the span                                                */
} sa_hip_token_docs;

typedef struct sa_hip_token_docs_info {
    uint64_t documents;     /* D; 0: the handle has no documents                                            */
    uint64_t bytes;         /* of starts, DA and PV: 8 n + 4 (D + 1)                                        */
    double   prepare_ms;    /* device time of the last set_documents: the three steps below                 */
    double   da_ms;         /* ... its document-array pass                                                  */
    double   sort_ms;       /* ... its sort of the ranks by document                                        */
    double   pv_ms;         /* ... its previous-rank pass                                                   */
    uint32_t sort_passes;   /* radix passes of that sort (0: one document)                                  */
    uint32_t reserved;      /* 0                                                                            */
    uint64_t locate_q;      /* spans of the last locate launch                                              */
    double   locate_ms;     /* HIP-event time of it (the call waits for it)                                 */
    uint64_t docs_q;        /* spans of the last documents launch                                           */
    double   docs_ms;       /* HIP-event time of it                                                         */
    uint64_t examined;      /* sum of its heads' examined: the ranks that launch streamed                   */
} sa_hip_token_docs_info;

int sa_hip_token_index_set_documents(sa_hip_token_index* t, const int32_t* doc_starts_host, uint32_t D);
/* Copy DA and PV of the ranks [first, first + count) to the host; either output may be NULL.  first + count > n and a handle
 * without documents return -1. */
int sa_hip_token_index_get_doc_range(sa_hip_token_index* t, uint64_t first, uint64_t count, int32_t* docs_out, int32_t* prev_out);
int sa_hip_token_index_docs_info(const sa_hip_token_index* t, sa_hip_token_docs_info* out);
/* spans_dev: sa_hip_token_span[Q]; docs_dev, offsets_dev: int32[Q * cap]; heads_dev: sa_hip_token_locate[Q]. */
int sa_hip_token_index_locate_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap, void* docs_dev,
                                           void* offsets_dev, void* heads_dev);
/* Both steps from host patterns: spans (may be NULL), docs, offs and heads out. */
int sa_hip_token_index_locate_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, uint32_t cap,
                                    sa_hip_token_span* spans, int32_t* docs, int32_t* offs, sa_hip_token_locate* heads);
/* heads_dev: sa_hip_token_docs[Q]; docs_dev and offsets_dev may be NULL when cap == 0. */
int sa_hip_token_index_docs_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap, uint32_t budget,
                                         void* docs_dev, void* offsets_dev, void* heads_dev);
int sa_hip_token_index_docs_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                  uint32_t max_length, int need_next, uint32_t cap, uint32_t budget, sa_hip_token_span* spans,
                                  int32_t* docs, int32_t* offs, sa_hip_token_docs* heads);

/* (6e) per-document counts and documents holding all n-grams of a group (csrc/token_all.hpp, csrc/capi_token_all.hpp): how often
 * an n-gram occurs in a given document (its term frequency), and which documents hold every n-gram of a group (an AND query).  All
 * results are exact.
 *
 * Both rest on one more array beside DA and PV of (6d), opt-in, 4 bytes per token: the rank-by-document array RK, int32[n], in which
 * RK[starts[d] .. starts[d + 1]) holds the ranks { r : DA[r] == d } in ascending order (document d owns starts[d + 1] - starts[d]
 * text positions and every position is one suffix, so the closed starts table bounds the segments; an empty document has an empty
 * segment).  sa_hip_token_index_prepare_doc_ranks(t, 1) builds it from the DA the handle holds (a no-op when it is there),
 * (t, 0) frees it; replacing or removing the documents drops it and the caller prepares again.  A handle that never prepares it has
 * the bytes and the answers of (6d).
 *
 *   doc_counts  counts[i * cap + j] = the number of ranks of span i that belong to document docs[i * cap + j], for j below the
 *               row's length: written[i] (a uint32 per span, written_stride bytes apart: the `written` field of a
 *               sa_hip_token_docs[Q] or sa_hip_token_all[G] can be passed as it stands with the struct's size as the stride), or
 *               cap when written is NULL.  Slots at or beyond a row's length are neither read nor written.  A document id outside
 *               [0, D), a negative one included, gives 0.
 *   all         spans[S] are cut into G groups by group_offsets[G + 1] (a HOST array in both forms, copied by the call): it starts
 *               at 0, ends at S, and every group has 1 .. SA_HIP_TOKEN_ALL_MAX spans.  The driver of a group is its span with
 *               the smallest count, the lowest index on a tie.  examined = budget ? min(count, budget) : count ranks of the driver
 *               are walked from its `first`; a rank r among them is a candidate iff it is the first of its document there
 *               (PV[r] < first), and a candidate matches iff its document holds a rank of every other span of the group.  The
 *               first min(matched, cap) matches are written in the driver's rank order: docs[g * cap + j] the document and
 *               offsets[g * cap + j] the offset inside it of the driver's smallest-rank occurrence there.  cap == 0 counts only;
 *               docs and offsets may then be NULL and are never touched.  matched is the exact number of documents that hold all
 *               n-grams of the group iff examined == count.  A group with an empty span has an empty driver: everything is 0.
 * Slots beyond `written` are not written.
 *
 * Errors returned as -1 before any HIP call: a NULL handle or a NULL required pointer, a handle without documents, a handle
 * without RK (the message names sa_hip_token_index_prepare_doc_ranks), a bad group table (not starting at 0, not ending at S, an
 * empty group, a group above the maximum), cap == 0 in doc_counts, a written_stride that is below 4 or no multiple of 4, G * cap,
 * Q * cap or S >= 2^31, mode or need_next other than 0 / 1, and descending offsets; Q == 0 and G == 0 are no-ops returning 0.  The
 * device forms take the spans exactly as sa_hip_token_index_spans_batch_device writes them and docs / written exactly as
 * sa_hip_token_index_docs_batch_device writes them, chain without a host trip and are asynchronous until sa_hip_token_index_sync;
 * they trust nothing: first and count are clamped to the array, every search is bounded.  The host forms run the span step first
 * and stage through buffers of the handle. */
#define SA_HIP_TOKEN_ALL_MAX 16

typedef struct sa_hip_token_all {
    uint32_t written;      /* entries written for this group: min(matched, cap)                    */
    uint32_t examined;     /* ranks of the driver walked: budget ? min(count, budget) : count      */
    uint32_t matched;      /* candidates whose document holds every other span of the group        */
    uint32_t candidates;   /* distinct documents among the examined ranks of the driver            */
    uint32_t driver;       /* index inside the group of the span that was walked                   */
    uint32_t count;        /* suffixes of the driver                                               */
    uint32_t reserved[2];  /* 0                                                                    */
} sa_hip_token_all;

typedef struct sa_hip_token_doc_ranks_info {
    uint32_t present;       /* 1: the handle holds RK                                              */
    uint32_t sort_passes;   /* radix passes of its sort (0: one document)                          */
    uint64_t bytes;         /* of RK: 4 n (0 when it is not there)                                 */
    double   prepare_ms;    /* device time of the last prepare that built it                       */
    uint64_t counts_q;      /* spans of the last doc_counts launch                                 */
    double   counts_ms;     /* HIP-event time of it (the call waits for it)                        */
    uint64_t all_q;         /* groups of the last all launch                                       */
    double   all_ms;        /* HIP-event time of it                                                */
} sa_hip_token_doc_ranks_info;

int sa_hip_token_index_prepare_doc_ranks(sa_hip_token_index* t, int on);
/* Copy RK[first .. first + count) to the host; first + count > n, a handle without documents or without RK return -1. */
int sa_hip_token_index_get_doc_ranks(sa_hip_token_index* t, uint64_t first, uint64_t count, int32_t* out);
int sa_hip_token_index_doc_ranks_info(const sa_hip_token_index* t, sa_hip_token_doc_ranks_info* out);
/* spans_dev: sa_hip_token_span[Q]; docs_dev: int32[Q * cap]; written_dev: NULL or a uint32 per span, written_stride bytes apart;
 * counts_dev: uint32[Q * cap]. */
int sa_hip_token_index_doc_counts_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t cap,
                                               const void* docs_dev, const void* written_dev, uint64_t written_stride,
                                               void* counts_dev);
/* Both steps from host patterns: docs int32[Q * cap] and written uint32[Q] (may be NULL) in, counts uint32[Q * cap] and spans (may
 * be NULL) out. */
int sa_hip_token_index_doc_counts_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                        uint32_t max_length, int need_next, uint32_t cap, const int32_t* docs,
                                        const uint32_t* written, uint32_t* counts, sa_hip_token_span* spans);
/* spans_dev: sa_hip_token_span[S]; group_offsets_host: uint64[G + 1]; docs_dev, offsets_dev: int32[G * cap] (may be NULL when
 * cap == 0); heads_dev: sa_hip_token_all[G]. */
int sa_hip_token_index_all_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t S, const uint64_t* group_offsets_host,
                                        uint64_t G, uint32_t cap, uint32_t budget, void* docs_dev, void* offsets_dev, void* heads_dev);
/* Both steps from S host patterns: spans[S] (may be NULL), docs, offs and heads[G] out. */
int sa_hip_token_index_all_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t S,
                                 const uint64_t* group_offsets, uint64_t G, int mode, uint32_t max_length, int need_next,
                                 uint32_t cap, uint32_t budget, sa_hip_token_span* spans, int32_t* docs, int32_t* offs,
                                 sa_hip_token_all* heads);

/* (6m) CNF document queries (csrc/token_cnf.hpp, csrc/capi_token_cnf.hpp): which documents satisfy an AND of clauses, every clause
 * an OR of n-grams, some clauses negated -- "(`New York` OR `NYC`) AND `subway`, but not `boilerplate`".  The AND query of (6e) is
 * its case of one literal per clause; it stays on its own kernel.  Needs the documents of (6d) and RK of (6e).  All results are exact.
 *
 * spans[S] are the literals.  The HOST table clause_offsets[C + 1] cuts them into C clauses, the HOST table group_offsets[G + 1] cuts
 * the clauses into G groups, one query per group; negated[C] (HOST, uint8; NULL: no clause is negated) marks clause c as an exclusion
 * with 1.  All three are copied by the call.  Every clause has >= 1 literal, every group has 1 .. SA_HIP_TOKEN_CNF_MAX_CLAUSES clauses,
 * at most SA_HIP_TOKEN_CNF_MAX_LITERALS literals and at least one clause that is not negated.
 *
 * A document MATCHES a group iff for every positive clause it holds a rank of at least one of the clause's literals, and for every
 * negated clause it holds a rank of none of its literals.
 *
 *   driver      the positive clause with the smallest sum of its literals' counts (formed in 64 bits), the lowest clause index on a
 *               tie.  A negated clause is never the driver, whatever its sum.  `count` is that sum.  A positive clause whose literals
 *               are all empty has the sum 0 and is therefore the driver: written, matched, candidates, duplicates, examined and count
 *               are 0 then (driver and literals still name the clause), as in (6e).
 *   walk        examined = budget ? min(count, budget) : count ranks.  The driver's literals are walked in literal order, each from
 *               its own `first`, and the budget is consumed in that order: an earlier literal is walked whole before a later one
 *               starts.  A walked rank r of literal l = [a_l, ..) is a first occurrence iff PV[r] < a_l.  A first occurrence is a
 *               duplicate iff its document holds a rank of an earlier literal l' < l of the driver clause (of that literal's WHOLE
 *               range: l' was walked whole before l began, so the document was listed there); otherwise it is a candidate.  The candidates are exactly the distinct documents of the
 *               union of the walked pieces, each at its first literal and there at its smallest rank.
 *   match       a candidate matches iff every other clause is satisfied.  Clauses are probed in clause order, literals in literal
 *               order; a positive clause stops at its first literal that holds the document, a negated one fails at it.
 *   output      the first min(matched, cap) matches in literal order, then rank order: docs[g * cap + j] the document and
 *               offsets[g * cap + j] = SA[r] - starts[doc] for the rank r that made it a candidate.  cap == 0 counts only; docs and
 *               offsets may then be NULL and are never touched.  Slots beyond `written` are not written.  matched is the exact
 *               number of matching documents iff examined == count.  (duplicates is a count of up to 63 first occurrences per
 *               document and is kept modulo 2^32.)
 *
 * `written` comes first in the head, so heads_dev chains into sa_hip_token_index_doc_counts_batch_device as written_dev with the
 * stride sizeof(sa_hip_token_cnf) = 48.
 *
 * Errors returned as -1 before any HIP call, the message naming the call: those (6e) lists for `all` -- a NULL handle or a NULL
 * required pointer, a handle without documents or without RK, mode or need_next other than 0 / 1, descending offsets, G * cap, S, C or
 * G >= 2^31 --, a clause table that does not start at 0 or end at S or holds an empty clause, a group table that does not start at 0
 * or end at C or holds an empty group, a group of more than 16 clauses or more than 64 literals, a group with no positive clause, a
 * negated byte other than 0 / 1.  G == 0 with good arguments is a no-op returning 0.  The device form takes the spans exactly as
 * sa_hip_token_index_spans_batch_device writes them (any rank range is a literal) and is asynchronous until sa_hip_token_index_sync;
 * it trusts nothing on the device: spans are clamped, group and clause sizes are clamped, every search is bounded.  The host form
 * runs the span step first and stages through buffers of the handle. */
#define SA_HIP_TOKEN_CNF_MAX_CLAUSES 16
#define SA_HIP_TOKEN_CNF_MAX_LITERALS 64

typedef struct sa_hip_token_cnf {
    uint32_t written;     /* min(matched, cap)                                                     */
    uint32_t matched;     /* candidates that satisfy every other clause                            */
    uint32_t candidates;  /* distinct documents among the examined ranks of the driver clause      */
    uint32_t duplicates;  /* first occurrences whose document an earlier literal of the driver has */
    uint32_t driver;      /* index inside the group of the clause that was walked                  */
    uint32_t literals;    /* literals of that clause                                               */
    uint64_t examined;    /* ranks walked: budget ? min(count, budget) : count                     */
    uint64_t count;       /* sum of the driver's literal counts                                    */
    uint64_t reserved;    /* 0                                                                     */
} sa_hip_token_cnf;

typedef struct sa_hip_token_cnf_info {
    uint64_t q;           /* groups of the last cnf launch                                         */
    double   ms;          /* HIP-event time of it                                                  */
} sa_hip_token_cnf_info;

/* spans_dev: sa_hip_token_span[S]; clause_offsets_host: uint64[C + 1]; negated_host: uint8[C] or NULL; group_offsets_host:
 * uint64[G + 1]; docs_dev, offsets_dev: int32[G * cap] (may be NULL when cap == 0); heads_dev: sa_hip_token_cnf[G]. */
int sa_hip_token_index_cnf_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t S,
                                        const uint64_t* clause_offsets_host, uint64_t C, const uint8_t* negated_host,
                                        const uint64_t* group_offsets_host, uint64_t G, uint32_t cap, uint32_t budget,
                                        void* docs_dev, void* offsets_dev, void* heads_dev);
/* Both steps from S host patterns: spans[S] (may be NULL), docs, offs and heads[G] out. */
int sa_hip_token_index_cnf_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t S,
                                 const uint64_t* clause_offsets, uint64_t C, const uint8_t* negated, const uint64_t* group_offsets,
                                 uint64_t G, int mode, uint32_t max_length, int need_next, uint32_t cap, uint32_t budget,
                                 sa_hip_token_span* spans, int32_t* docs, int32_t* offs, sa_hip_token_cnf* heads);
int sa_hip_token_index_cnf_info(const sa_hip_token_index* t, sa_hip_token_cnf_info* out);

/* (6f) matching statistics (csrc/token_match.hpp, csrc/capi_token_match.hpp): which parts of a query text stand verbatim in the
 * corpus.  For every position of the text the longest prefix of what follows that the corpus holds, with its range and count, and
 * per query document the maximal matches, the longest one and the tokens they cover.  All results are exact.
 *
 * A batch is Q query documents in the usual layout: document d is patterns[offsets[d] .. offsets[d + 1]), the offsets are
 * non-decreasing.  A position is a flat index j into patterns; total = offsets[Q].  With M = max_length (0: no cap) and avail(j) =
 * the tokens from j to the end of j's document:
 *   ms(j)   the largest L <= min(avail(j), M, n) such that patterns[j .. j + L) occurs in the text;
 *   match   spans[j] = {first, count, length = ms(j), ended} of that prefix: exactly what sa_hip_token_index_spans_batch answers in
 *           mode 0 for it.  L = 0 gives {0, n, 0, 0}; with n == 0 every match is {0, 0, 0, 0}; a position outside every document
 *           (j < offsets[0]) gets {0, 0, 0, 0};
 *   end(j)  j + ms(j); it never passes the end of j's document and is non-decreasing in j.
 * A match of length >= 1 is maximal when no other position's match of the same document contains it, which holds iff
 * end(j) > end(j - 1).  Per document the docs step gives the maximal matches of at least min_length (>= 1) symbols in position
 * order: positions[d * cap + k] = the offset inside the document, out_spans[d * cap + k] = its match, for k < written; and the head
 * {written = min(maximal, cap), maximal = how many there are, longest = the largest ms of the document whatever min_length is,
 * covered = the tokens of the document that lie inside a match of at least min_length symbols}.  Cells beyond `written` are not
 * written; cap == 0 computes the heads alone, positions and out_spans may then be NULL and are never touched; an empty document has
 * a head of zeros.
 *
 * Cost: a position is one range search, two comparisons against its neighbours in suffix order and, where 1 <= ms(j) < the capped
 * length, a second range search; a search step compares as many symbols as its suffix shares with the text, so a text copied
 * verbatim from the corpus costs about m * min(m, M) * log2 n symbol reads for its m positions.  max_length is the caller's lever.
 *
 * Errors returned as -1 before any HIP call: a NULL handle or a NULL required pointer, min_length == 0, total >= 2^31,
 * Q * cap >= 2^31, and in the host forms (which compute total) descending offsets; Q == 0 is a no-op returning 0; no usable device
 * -3.  The device forms are asynchronous on the handle's stream until sa_hip_token_index_sync and chain without a host trip (the
 * span output of the first is the span input of the second); they trust nothing: every loop is bounded, a document's end is
 * clamped to total, a span's length to what is left of its document, and an array that is not the suffix array gives unspecified
 * answers.  The host forms stage through buffers of the handle and copy out only the written cells of a row. */
typedef struct sa_hip_token_match_head {
    uint32_t written;    /* maximal matches written for this document: min(maximal, cap)        */
    uint32_t maximal;    /* maximal matches of at least min_length symbols                       */
    uint32_t longest;    /* the largest ms(j) of the document                                    */
    uint32_t covered;    /* tokens inside a match of at least min_length symbols                 */
} sa_hip_token_match_head;

typedef struct sa_hip_token_match_info {
    uint64_t q;            /* documents of the last launch of either kind                        */
    uint64_t positions;    /* positions of the last match launch                                 */
    double   match_ms;     /* HIP-event time of the last match launch (the call waits for it)    */
    double   docs_ms;      /* ... of the last docs launch                                        */
} sa_hip_token_match_info;

/* spans_dev: sa_hip_token_span[total], total = offsets[Q], index = position in patterns. */
int sa_hip_token_index_match_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                          uint64_t total, uint32_t max_length, void* spans_dev);
/* spans_dev as the call above writes them; positions_dev: uint32[Q * cap] and out_spans_dev: sa_hip_token_span[Q * cap] (may be
 * NULL when cap == 0); heads_dev: sa_hip_token_match_head[Q]. */
int sa_hip_token_index_match_docs_batch_device(sa_hip_token_index* t, const void* spans_dev, const void* offsets_dev, uint64_t Q,
                                               uint32_t min_length, uint32_t cap, void* positions_dev, void* out_spans_dev,
                                               void* heads_dev);
/* Host pointers; spans[offsets[Q]] out. */
int sa_hip_token_index_match_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                   uint32_t max_length, sa_hip_token_span* spans);
/* Both steps from host documents: spans[offsets[Q]] (may be NULL), positions, out_spans and heads[Q] out. */
int sa_hip_token_index_match_docs_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                        uint32_t max_length, uint32_t min_length, uint32_t cap, sa_hip_token_span* spans,
                                        uint32_t* positions, sa_hip_token_span* out_spans, sa_hip_token_match_head* heads);
int sa_hip_token_index_match_info(const sa_hip_token_index* t, sa_hip_token_match_info* out);

/* (6c, matching statistics) the calls of (6f) over a shard set (csrc/token_shard_match.hpp, csrc/capi_token_shard_match.hpp).  The
 * batch layout, M = max_length, avail(j), the flat positions and total = offsets[Q] are those of (6f); n_s is the length of shard s.
 *   ms(j)      the largest L <= min(avail(j), M) such that patterns[j .. j + L) occurs in SOME shard: the maximum over s of what
 *              shard s's own sa_hip_token_index_match_batch answers for j.  Shards are cut at document boundaries and a match never
 *              spans a cut, so this is the matching statistic of the corpus as the set defines it; end(j) = j + ms(j) is
 *              non-decreasing and a match is maximal iff end(j) > end(j - 1), as in (6f);
 *   per_shard  [s * total + j], shard-major like every per-shard array of the set: what shard s's own spans_batch answers in mode 0
 *              for patterns[j .. j + ms(j)) -- count 0 with the exact lower bound where the shard does not hold it, {first, 1, L, 1}
 *              where it only ends the shard's text, {0, n_s, 0, 0} for L = 0, zeros from an empty shard and, in every shard, for a
 *              position outside every document (j < offsets[0]);
 *   merged     [j] = {length = ms(j), shards = how many shards have a count > 0, count = the sum over s of the per-shard counts};
 *              a position outside every document, or a set of empty shards, gives zeros;
 *   docs step  over merged, as in (6f): positions[d * cap + k] the offset inside the document, out_matches[d * cap + k] the merged
 *              record of the k-th maximal match of at least min_length (>= 1) symbols, the head as in (6f).  Cells beyond `written`
 *              are not written; cap == 0 computes the heads alone and touches neither array; an empty document has a head of zeros.
 * With S == 1 length, count, per_shard, positions and heads equal the single index's answers.
 *
 * A position costs one range search and two neighbour comparisons per shard, then one more range search in every shard but the
 * one that found the whole capped prefix.  The searches of a position's S shards run in neighbouring lanes.
 *
 * Errors returned as -1 before the set is dereferenced and before any HIP call: a NULL set or a NULL required pointer,
 * min_length == 0, total >= 2^31, Q * cap >= 2^31, and in the host forms (which compute total) descending offsets; Q == 0 is a
 * no-op returning 0; no usable device -3.  The device forms are asynchronous on the set's stream until sa_hip_token_shards_sync
 * and chain without a host trip: merged_dev of the first is the input of the second, and per_shard_dev (required there,
 * sa_hip_token_span[S * total]) has the layout of the set's span output with Q = total, so sa_hip_token_shards_next_batch_device(set,
 * per_shard_dev, total, cap, ...) gives the tokens that follow the longest match at every position.  They trust nothing: every loop
 * is bounded, a document's end is clamped to total, a length to what is left of its document.  A scratch of S * total uint32 belongs
 * to the set and grows on demand.  The host forms stage through buffers of the set and copy out only the written cells of a row;
 * per_shard (match_batch) and merged (match_docs_batch) are copied back only when given. */
typedef struct sa_hip_token_shards_match {
    uint32_t length;    /* ms(j): the longest match over all shards                            */
    uint32_t shards;    /* shards that hold it (count > 0)                                     */
    uint64_t count;     /* its occurrences over all shards                                     */
} sa_hip_token_shards_match;

typedef struct sa_hip_token_shards_match_stats {
    uint64_t q;            /* documents of the last launch of either kind                        */
    uint64_t positions;    /* positions of the last match launches                               */
    double   match_ms;     /* HIP-event time of the last three match launches together           */
    double   docs_ms;      /* ... of the last docs launch                                        */
} sa_hip_token_shards_match_stats;

/* merged_dev: sa_hip_token_shards_match[total]; per_shard_dev: sa_hip_token_span[S * total]; total = offsets[Q]. */
int sa_hip_token_shards_match_batch_device(sa_hip_token_shards* set, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           uint64_t total, uint32_t max_length, void* merged_dev, void* per_shard_dev);
/* merged_dev as the call above writes it; positions_dev: uint32[Q * cap] and out_matches_dev: sa_hip_token_shards_match[Q * cap]
 * (may be NULL when cap == 0); heads_dev: sa_hip_token_match_head[Q]. */
int sa_hip_token_shards_match_docs_batch_device(sa_hip_token_shards* set, const void* merged_dev, const void* offsets_dev, uint64_t Q,
                                                uint32_t min_length, uint32_t cap, void* positions_dev, void* out_matches_dev,
                                                void* heads_dev);
/* Host pointers; merged[offsets[Q]] out, per_shard[S * offsets[Q]] out or NULL. */
int sa_hip_token_shards_match_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    uint32_t max_length, sa_hip_token_shards_match* merged, sa_hip_token_span* per_shard);
/* Both steps from host documents: merged[offsets[Q]] (may be NULL), positions, out_matches and heads[Q] out. */
int sa_hip_token_shards_match_docs_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                         uint32_t max_length, uint32_t min_length, uint32_t cap, sa_hip_token_shards_match* merged,
                                         uint32_t* positions, sa_hip_token_shards_match* out_matches, sa_hip_token_match_head* heads);
int sa_hip_token_shards_match_info(const sa_hip_token_shards* set, sa_hip_token_shards_match_stats* out);

/* (6g) documents over a shard set (csrc/token_shard_docs.hpp, csrc/capi_token_shard_docs.hpp): the calls of (6d) answered for the
 * whole corpus.  All results are exact.
 *
 * The set is one corpus cut at document boundaries, so a document lives in exactly one shard.  With D_s documents in shard s, empty
 * ones included, base[0] = 0 and base[s + 1] = base[s] + D_s; the global id of document d of shard s is base[s] + d, a uint64.  The
 * hits of a context are the concatenation of the shards' rank ranges in shard order, suffix order inside a shard.  For context i the
 * span step of the set gives spans[s * Q + i]; c_s is its count clamped to the shard and C = the sum of the c_s, a uint64.
 *
 *   locate  the first min(C, cap) hits of that concatenation as (global document, offset inside it) to docs[i * cap ..] and
 *           offsets[i * cap ..]; the head is {written, count = C}.
 *   docs    examined = budget ? min(C, budget) : C ranks are taken from the front of the concatenation: shard s examines
 *           e_s = clamp(budget - (c_0 + .. + c_(s-1)), 0, c_s) ranks of its span, c_s without a budget.  distinct = the sum over s
 *           of the distinct documents among those e_s ranks -- two shards never share a document, so nothing is de-duplicated
 *           across them.  The list is the shards' lists of (6d) one after another, global ids, cut at cap.  The head is {written =
 *           min(distinct, cap), examined, distinct, count = C}; distinct is the exact document frequency iff examined == count.
 *           cap == 0 counts only; docs and offsets may then be NULL and are never touched.
 * Slots beyond `written` are not written.  With S == 1 every answer equals the single index's, the document ids widened.
 *
 * sa_hip_token_shards_set_documents gives every shard its table through sa_hip_token_index_set_documents: starts[s] is the table
 * of shard s, D[s] >= 1 its length, every entry required; all S tables are checked by the rules of (6d) before the first shard is
 * touched.  NULL starts and NULL D remove the documents from all shards.  sa_hip_token_shards_adopt_documents builds the set's
 * table from documents the shards already have (set through the borrowed handle, or before the handle joined the set); -1 if a
 * shard has none.  A shard's documents can be replaced behind the set's back through sa_hip_token_shards_shard: every handle
 * counts its set_documents calls, and every call below compares the counts the set recorded before any launch; where they differ
 * it returns -1 and the message names sa_hip_token_shards_adopt_documents.  As with every use of a borrowed handle, the caller
 * synchronises the set before it changes a shard.
 *
 * The per-shard lists of the docs calls live in scratch of the set, S * cap * 8 bytes plus 16 per shard and context (the heads
 * alone when cap == 0), worked through in chunks of contexts exactly as the next-symbol calls of (6c) are.
 *
 * Errors returned as -1 before any HIP call: those of (6c) and (6d) -- a NULL set or a NULL required pointer, mode or need_next
 * other than 0 / 1, cap == 0 in locate, Q * cap >= 2^31, descending offsets -- and a set without documents or whose shards'
 * documents changed; Q == 0 is a no-op returning 0.  The device forms take sa_hip_token_span[S * Q] exactly as
 * sa_hip_token_shards_spans_batch_device writes them, chain with it without a host trip and are asynchronous until
 * sa_hip_token_shards_sync; they trust nothing: first and count are clamped to the shard, every loop is bounded.  The host forms
 * run the span step first (locate always in mode 0) and stage through buffers of the set. */
typedef struct sa_hip_token_shards_locate {
    uint32_t written;    /* entries written for this context: min(count, cap)                   */
    uint32_t reserved;   /* 0                                                                   */
    uint64_t count;      /* hits over all shards                                                */
} sa_hip_token_shards_locate;

typedef struct sa_hip_token_shards_docs {
    uint32_t written;    /* entries written for this context: min(distinct, cap)                */
    uint32_t reserved;   /* 0                                                                   */
    uint64_t examined;   /* ranks walked over all shards: budget ? min(count, budget) : count   */
    uint64_t distinct;   /* distinct documents among them                                       */
    uint64_t count;      /* hits over all shards                                                */
} sa_hip_token_shards_docs;

typedef struct sa_hip_token_shards_docs_stats {
    uint64_t documents;    /* of the set: base[S]; 0: the set has no documents                             */
    uint32_t chunk;        /* contexts per chunk of the last docs call (0: none yet)                       */
    uint32_t reserved;     /* 0                                                                            */
    uint64_t locate_q;     /* contexts of the last locate launch                                           */
    double   locate_ms;    /* HIP-event time of it (the call waits for it)                                 */
    uint64_t pairs_q;      /* (context, shard) pairs of the last docs call                                 */
    double   pairs_ms;     /* HIP-event time of its pair launches, over its chunks                         */
    uint64_t merge_q;      /* contexts of the last merge launches                                          */
    double   merge_ms;     /* HIP-event time of them, over the chunks                                      */
    uint64_t streamed;     /* sum of the pairs' examined: the ranks the last docs call streamed            */
} sa_hip_token_shards_docs_stats;

/* starts[S] host tables, D[S] their lengths; both NULL: remove the documents. */
int sa_hip_token_shards_set_documents(sa_hip_token_shards* set, const int32_t* const* starts, const uint32_t* D);
int sa_hip_token_shards_adopt_documents(sa_hip_token_shards* set);
/* out: uint64[S + 1], base[S] = the documents of the set. */
int sa_hip_token_shards_doc_bases(sa_hip_token_shards* set, uint64_t* out);
int sa_hip_token_shards_docs_info(const sa_hip_token_shards* set, sa_hip_token_shards_docs_stats* out);
/* spans_dev: sa_hip_token_span[S * Q]; docs_dev: uint64[Q * cap]; offsets_dev: int32[Q * cap]; heads_dev:
 * sa_hip_token_shards_locate[Q]. */
int sa_hip_token_shards_locate_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t Q, uint32_t cap, void* docs_dev,
                                            void* offsets_dev, void* heads_dev);
/* Both steps from host patterns: spans[S * Q] (may be NULL), docs, offs and heads out. */
int sa_hip_token_shards_locate_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                     uint32_t cap, sa_hip_token_span* spans, uint64_t* docs, int32_t* offs,
                                     sa_hip_token_shards_locate* heads);
/* heads_dev: sa_hip_token_shards_docs[Q]; docs_dev and offsets_dev may be NULL when cap == 0. */
int sa_hip_token_shards_docs_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t Q, uint32_t cap, uint64_t budget,
                                          void* docs_dev, void* offsets_dev, void* heads_dev);
int sa_hip_token_shards_docs_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q, int mode,
                                   uint32_t max_length, int need_next, uint32_t cap, uint64_t budget, sa_hip_token_span* spans,
                                   uint64_t* docs, int32_t* offs, sa_hip_token_shards_docs* heads);
/* The last step of the two calls above on its own: S lists per context as the pair launch writes them -- docs_dev int32[S * Q * cap]
 * (row (s * Q + i) * cap, ids local to the shard), offsets_dev int32[S * Q * cap], heads_dev sa_hip_token_docs[S * Q] (written is
 * clamped to cap) -- into out_docs_dev uint64[Q * cap], out_offsets_dev int32[Q * cap], out_heads_dev sa_hip_token_shards_docs[Q].
 * bases_dev: uint64[S + 1] on the device, or NULL for the set's own (which needs the set's documents).  With cap == 0 the four list
 * pointers may be NULL.  Asynchronous on the set's stream. */
int sa_hip_token_shards_docs_merge_device(sa_hip_token_shards* set, const void* docs_dev, const void* offsets_dev, const void* heads_dev,
                                          const void* bases_dev, uint64_t Q, uint32_t cap, void* out_docs_dev, void* out_offsets_dev,
                                          void* out_heads_dev);

/* (6h) per-document counts and AND groups over a shard set (csrc/token_shard_all.hpp, csrc/capi_token_shard_all.hpp): the calls of
 * (6e) answered for the whole corpus of (6g).  All results are exact.
 *
 * Notation of (6g): S shards, base[s] the global id of shard s's first document, a document lives in one shard.  P patterns have the
 * spans spans[s * P + p] as sa_hip_token_shards_spans_batch_device writes them; c_{s,p} is the count clamped to shard s and
 * C_p = the sum of the c_{s,p}, a uint64.
 *
 * Every shard carries RK of (6e).  sa_hip_token_shards_prepare_doc_ranks(set, 1) calls sa_hip_token_index_prepare_doc_ranks for
 * every shard, one after another (the sort scratch, 24 n_s bytes, is held for one shard at a time; a no-op per shard where RK is
 * there), then builds the set's table of the shards' arrays; (set, 0) frees RK in all shards and drops the table.  A set without
 * documents returns -1.  RK of a shard can be freed or rebuilt through sa_hip_token_shards_shard: every handle counts the
 * prepare_doc_ranks calls that build or free and the drops caused by set_documents, and every call below compares the counts the set
 * recorded -- beside the document counts of (6g) -- before any launch; where they differ it returns -1 and the message names
 * sa_hip_token_shards_prepare_doc_ranks (sa_hip_token_shards_adopt_documents for the documents).  (set, 1) again re-adopts.
 *
 *   doc_counts  counts[i * cap + j] = the number of ranks of context i's spans that belong to the document with the global id
 *               docs[i * cap + j] (uint64), for j below the row's length: written[i] (a uint32 per context, written_stride bytes
 *               apart: the `written` field of a sa_hip_token_shards_docs[Q] or sa_hip_token_shards_all[G] can be passed as it stands
 *               with the struct's size as the stride), or cap when written is NULL.  Global id g lives in the shard s with
 *               base[s] <= g < base[s + 1]; its count is that of (6e) for document g - base[s] of that shard against
 *               spans[s * Q + i], a uint32.  An id >= base[S] gives 0.  Slots at or beyond a row's length are neither read nor
 *               written.
 *   all         the P patterns are cut into G groups by group_offsets[G + 1] (a HOST array in both forms, copied by the call) under
 *               the rules of (6e).  The driver of a group is its pattern with the smallest C_j over ALL shards, the lowest index on
 *               a tie: one driver per group, not one per shard.  examined = budget ? min(C_driver, budget) : C_driver ranks are
 *               taken from the front of the concatenation of the driver's ranges in shard order: shard s examines
 *               e_s = clamp(budget - (c_{0,driver} + .. + c_{s-1,driver}), 0, c_{s,driver}) ranks.  Per shard the candidates and
 *               the matches are those of (6e) over these e_s ranks, probing the group's other spans of the same shard; matched and
 *               candidates are the plain sums over the shards (two shards never share a document).  The list is the shards' lists
 *               one after another, each in the driver's rank order, global ids, every entry with the offset of the driver's
 *               smallest-rank occurrence in that document, cut at cap.  cap == 0 counts only; docs and offsets may then be NULL
 *               and are never touched.  matched is the exact number of documents that hold all n-grams of the group iff
 *               examined == count.  A group whose driver is empty has an all-zero head apart from `driver`.
 * Slots beyond `written` are not written.  With S == 1 every answer equals the single index's, the document ids widened.
 *
 * The per-pair lists of the all calls live in scratch of the set, S * cap * 8 bytes plus 16 per shard and group (the heads and the
 * plan alone when cap == 0), worked through in chunks of groups exactly as the docs calls of (6g) are.
 *
 * Errors returned as -1 before any HIP call: those of (6e) and (6g) -- a NULL set or a NULL required pointer, a set without
 * documents or whose shards' documents changed, a bad group table, cap == 0 in doc_counts, a written_stride below 4 or no multiple
 * of 4, mode or need_next other than 0 / 1, descending offsets -- a set without rank arrays (the message names
 * sa_hip_token_shards_prepare_doc_ranks), rank arrays that changed behind the set, and P, G * cap or Q * cap >= 2^31; Q == 0 and
 * G == 0 are no-ops returning 0.  The device forms chain with sa_hip_token_shards_spans_batch_device and
 * sa_hip_token_shards_docs_batch_device without a host trip and are asynchronous until sa_hip_token_shards_sync; they trust nothing:
 * first and count are clamped to the shard, every search and every loop is bounded.  The host forms run the span step first (in
 * mode 1 it gives one length per context for all shards, so a group's n-grams are the same in every shard) and stage through buffers
 * of the set. */
typedef struct sa_hip_token_shards_all {
    uint32_t written;      /* entries written for this group: min(matched, cap)                          */
    uint32_t driver;       /* index inside the group of the pattern that was walked                      */
    uint64_t examined;     /* ranks of the driver walked over all shards: budget ? min(count, budget) : count */
    uint64_t matched;      /* candidates whose document holds every other n-gram of the group            */
    uint64_t candidates;   /* distinct documents among the examined ranks of the driver                  */
    uint64_t count;        /* occurrences of the driver over all shards                                  */
} sa_hip_token_shards_all;

typedef struct sa_hip_token_shards_ranks_stats {
    uint32_t present;      /* 1: the set holds a table of its shards' RK                                   */
    uint32_t chunk;        /* groups per chunk of the last all call (0: none yet)                          */
    uint64_t bytes;        /* of the shards' RK, summed                                                    */
    double   prepare_ms;   /* device time of the shards' last prepares, summed                             */
    uint64_t counts_q;     /* contexts of the last doc_counts launch                                       */
    double   counts_ms;    /* HIP-event time of it (the call waits for it)                                 */
    uint64_t plan_q;       /* groups of the last all call                                                  */
    double   plan_ms;      /* HIP-event time of its plan launches, over its chunks                         */
    uint64_t pairs_q;      /* (group, shard) pairs of the last all call                                    */
    double   pairs_ms;     /* HIP-event time of its pair launches, over its chunks                         */
    uint64_t merge_q;      /* groups of the last merge launches                                            */
    double   merge_ms;     /* HIP-event time of them, over the chunks                                      */
    uint64_t streamed;     /* sum of the pairs' examined: the ranks the last all call streamed             */
} sa_hip_token_shards_ranks_stats;

int sa_hip_token_shards_prepare_doc_ranks(sa_hip_token_shards* set, int on);
int sa_hip_token_shards_doc_ranks_info(const sa_hip_token_shards* set, sa_hip_token_shards_ranks_stats* out);
/* spans_dev: sa_hip_token_span[S * Q]; docs_dev: uint64[Q * cap]; written_dev: NULL or a uint32 per context, written_stride bytes
 * apart; counts_dev: uint32[Q * cap]. */
int sa_hip_token_shards_doc_counts_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t Q, uint32_t cap,
                                                const void* docs_dev, const void* written_dev, uint64_t written_stride,
                                                void* counts_dev);
/* Both steps from host patterns: docs uint64[Q * cap] and written uint32[Q] (may be NULL) in, counts uint32[Q * cap] and
 * spans[S * Q] (may be NULL) out. */
int sa_hip_token_shards_doc_counts_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                         int mode, uint32_t max_length, int need_next, uint32_t cap, const uint64_t* docs,
                                         const uint32_t* written, uint32_t* counts, sa_hip_token_span* spans);
/* spans_dev: sa_hip_token_span[S * P]; group_offsets_host: uint64[G + 1]; docs_dev: uint64[G * cap], offsets_dev: int32[G * cap]
 * (may be NULL when cap == 0); heads_dev: sa_hip_token_shards_all[G]. */
int sa_hip_token_shards_all_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t P,
                                         const uint64_t* group_offsets_host, uint64_t G, uint32_t cap, uint64_t budget,
                                         void* docs_dev, void* offsets_dev, void* heads_dev);
/* Both steps from P host patterns: spans[S * P] (may be NULL), docs, offs and heads[G] out. */
int sa_hip_token_shards_all_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t P,
                                  const uint64_t* group_offsets, uint64_t G, int mode, uint32_t max_length, int need_next,
                                  uint32_t cap, uint64_t budget, sa_hip_token_span* spans, uint64_t* docs, int32_t* offs,
                                  sa_hip_token_shards_all* heads);
/* The last step of the two calls above on its own: S lists per group as the pair launch writes them -- docs_dev int32[S * G * cap]
 * (row (s * G + g) * cap, ids local to the shard), offsets_dev int32[S * G * cap], heads_dev uint32[S * G][4] = {written (clamped
 * to cap), examined, matched, candidates} -- and plan_dev, per group {uint32 driver, uint32 0, uint64 count} as the plan launch
 * writes it, into out_docs_dev uint64[G * cap], out_offsets_dev int32[G * cap], out_heads_dev sa_hip_token_shards_all[G].
 * bases_dev: uint64[S + 1] on the device, or NULL for the set's own (which needs the set's documents).  With cap == 0 the four list
 * pointers may be NULL.  Needs no rank arrays.  Asynchronous on the set's stream. */
int sa_hip_token_shards_all_merge_device(sa_hip_token_shards* set, const void* docs_dev, const void* offsets_dev, const void* heads_dev,
                                         const void* plan_dev, const void* bases_dev, uint64_t G, uint32_t cap, void* out_docs_dev,
                                         void* out_offsets_dev, void* out_heads_dev);

/* (6i) infinity-gram scores (csrc/token_score.hpp, csrc/capi_token_score.hpp): the probability the corpus gives every token of a
 * query text under the model "the longest context that occurs, and what followed it".  For every position the length of that
 * context, how often it occurs with a token behind it, and how often that token is the one in the text; per query document the
 * sums a perplexity needs.  All results are exact; no floating point is computed on the device.
 *
 * The batch layout is that of (6f): Q query documents, document d = patterns[offsets[d] .. offsets[d + 1]), offsets non-decreasing,
 * a position a flat index j, total = offsets[Q], M = max_length (0: no cap), s(j) the start of j's document.  The effective count
 * of a context is count - ended as in mode 1 of (6b) with need_next = 1: its occurrences that have a token behind them; the empty
 * context has n.  For a position j inside a document, scores[j] =
 *   length         L(j): the largest L <= min(j - s(j), M, n) such that patterns[j - L .. j) has an effective count >= 1;
 *   context_count  that effective count: >= 1 whenever n >= 1;
 *   token_count    the occurrences of patterns[j - L .. j], the same context with the token at j appended: <= context_count, and 0
 *                  for a token outside the alphabet;
 *   first          the `first` of that (L + 1)-gram's range as sa_hip_token_index_query_batch gives it, exact also when token_count
 *                  is 0: {first, token_count, L + 1} is a span that sa_hip_token_index_locate_* and _next_* take.
 * The token's probability is token_count / context_count.  With n == 0 every record is {0, 0, 0, 0}, as is that of a position
 * outside every document (j < offsets[0]).  Per document the docs step gives the head {scored = its positions, seen = those with
 * token_count > 0, certain = those with token_count == context_count, longest = the largest length, length_sum = the sum of the
 * lengths}; an empty document has a head of zeros (and with n == 0, where every record is zero, certain == scored).
 *
 * spans_dev of the score call is NULL, or the matches sa_hip_token_index_match_batch_device wrote for the SAME batch and the SAME
 * max_length.  With them the start of the context comes from a binary search over these records and one range search (where the
 * context is the corpus's tail and occurs nowhere else, a search over the shorter contexts follows); without them, from a binary
 * search over L with one range search per probe.  Both give the same records, byte for byte.  The host form takes the first way
 * and runs the match launch itself, into a buffer of the handle.
 *
 * Cost: as in (6f) a search step compares as many symbols as its suffix shares with the context, so a text copied verbatim from
 * the corpus costs about m * min(m, M) * log2 n symbol reads for its m positions.  max_length is the caller's lever.
 *
 * Errors returned as -1 before any HIP call: a NULL handle or a NULL required pointer, total >= 2^31, in the host form descending
 * offsets and scores and heads both NULL; Q == 0 is a no-op returning 0; no usable device -3.  The device forms are asynchronous
 * on the handle's stream until sa_hip_token_index_sync and chain behind sa_hip_token_index_match_batch_device without a host trip;
 * they trust nothing: every loop is bounded, a context's start is clamped to its document and to the batch, and records that no
 * match launch wrote or an array that is not the suffix array give unspecified answers.  The host form stages through buffers of
 * the handle. */
typedef struct sa_hip_token_score {
    uint32_t length;          /* L(j): symbols of the context                                         */
    uint32_t context_count;   /* occurrences of the context that have a token behind them             */
    uint32_t token_count;     /* occurrences of the context followed by the token at j                */
    uint32_t first;           /* suffixes that sort before the context followed by the token at j     */
} sa_hip_token_score;

typedef struct sa_hip_token_score_head {
    uint32_t scored;          /* positions of the document                                            */
    uint32_t seen;            /* those with token_count > 0                                           */
    uint32_t certain;         /* those with token_count == context_count                              */
    uint32_t longest;         /* the largest length                                                   */
    uint64_t length_sum;      /* the sum of the lengths                                               */
} sa_hip_token_score_head;

typedef struct sa_hip_token_score_info {
    uint64_t q;               /* documents of the last launch of either kind                          */
    uint64_t positions;       /* positions of the last score launch                                   */
    double   match_ms;        /* HIP-event time of the last match launch (the call waits for it)      */
    double   score_ms;        /* ... of the last score launch                                         */
    double   docs_ms;         /* ... of the last score docs launch                                    */
} sa_hip_token_score_info;

/* spans_dev: NULL, or sa_hip_token_span[total] as sa_hip_token_index_match_batch_device wrote them for this batch and max_length;
 * scores_dev: sa_hip_token_score[total], total = offsets[Q], index = position in patterns. */
int sa_hip_token_index_score_batch_device(sa_hip_token_index* t, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                          uint64_t total, uint32_t max_length, const void* spans_dev, void* scores_dev);
/* scores_dev as the call above writes them (may be NULL when every document is empty); heads_dev: sa_hip_token_score_head[Q]. */
int sa_hip_token_index_score_docs_batch_device(sa_hip_token_index* t, const void* scores_dev, const void* offsets_dev, uint64_t Q,
                                               void* heads_dev);
/* Host pointers; scores[offsets[Q]] and heads[Q] out, either may be NULL, not both. */
int sa_hip_token_index_score_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                   uint32_t max_length, sa_hip_token_score* scores, sa_hip_token_score_head* heads);
int sa_hip_token_index_score_info(const sa_hip_token_index* t, sa_hip_token_score_info* out);

/* (6j) infinity-gram scores over a shard set (csrc/token_shard_score.hpp, csrc/capi_token_shard_score.hpp): the calls of (6i)
 * answered for the whole corpus of a set.  All results are exact; no floating point is computed on the device.
 *
 * The batch layout, M = max_length, s(j), the flat positions and total = offsets[Q] are those of (6i); S shards, n_s the length of
 * shard s, max_n the longest.  For a context C, eff_s(C) = count_s(C) - ended_s(C) is its effective count in shard s as in (6i)
 * (the empty context: n_s), and eff(C) the sum over the shards.  For a position j inside a document,
 *   scores[j]     length         L(j): the largest L <= min(j - s(j), M, max_n) such that eff(patterns[j - L .. j)) >= 1;
 *                 context_count  that eff: >= 1 whenever some shard is not empty;
 *                 token_count    the sum over s of the occurrences of patterns[j - L .. j] in shard s: <= context_count, and 0
 *                                for a token no shard holds behind the context;
 *                 shards         the shards whose own token_count is > 0;
 *   per_shard     [s * total + j], shard-major like every per-shard array of the set: what shard s's own spans_batch answers in
 *                 mode 0 for the (L(j) + 1)-gram patterns[j - L .. j] -- {first, count, L + 1, ended}, count 0 with the exact lower
 *                 bound where the shard does not hold it (also where it does not hold the context), zeros from an empty shard.
 * A position outside every document (j < offsets[0]) gives zeros in scores and in every shard's cell; a set of empty shards gives
 * zeros everywhere.  The token's probability is token_count / context_count.  The docs step gives the head of (6i) per document:
 * seen = its positions with token_count > 0, certain = those with token_count == context_count; an empty document has a head of
 * zeros.  With S == 1 length, context_count, token_count, per_shard[..].first / .count and the heads equal the single index's.
 *
 * The set defines its corpus as the shards' texts side by side: a context whose only occurrence in the concatenation lies across
 * a cut is not an occurrence, and the set answers a shorter L there than an unsharded index of the concatenation would.
 *
 * merged_dev of the score call is NULL, or the records sa_hip_token_shards_match_batch_device wrote for the SAME batch and the SAME
 * max_length.  With them the candidate context comes from a binary search over these records and one range search per shard; where
 * every shard that holds the candidate holds it only as the tail of its text (up to S shards can share a tail), a search over the
 * shorter contexts follows.  Without them that search starts from the capped context.  Both give the same records, byte for byte.
 * The host form takes the first way and runs the match launches itself, into buffers of the set.
 *
 * Errors returned as -1 before the set is dereferenced and before any HIP call: a NULL set or a NULL required pointer,
 * total >= 2^31, in the host form descending offsets and scores, per_shard and heads all NULL; Q == 0 is a no-op returning 0; no
 * usable device -3.  (S <= 64 and total < 2^31 keep the S * total lanes of a launch below 2^31 workgroups; the launch tests it all
 * the same.)  The device forms are asynchronous on the set's stream until sa_hip_token_shards_sync and chain behind
 * sa_hip_token_shards_match_batch_device without a host trip; per_shard_dev (required, sa_hip_token_span[S * total]) has the layout
 * of the set's span output with Q = total, so sa_hip_token_shards_next_batch_device, _locate_batch_device and _docs_batch_device
 * take it as it is.  They trust nothing: every loop is bounded, a context's start is clamped to its document and to the batch.  A
 * scratch of 3 * S * total uint32 belongs to the set and grows on demand. */
typedef struct sa_hip_token_shards_score {
    uint32_t length;          /* L(j): symbols of the context                                         */
    uint32_t shards;          /* shards that hold the context followed by the token at j              */
    uint64_t context_count;   /* occurrences of the context over all shards with a token behind them  */
    uint64_t token_count;     /* occurrences of the context followed by the token at j, over all      */
} sa_hip_token_shards_score;

typedef struct sa_hip_token_shards_score_stats {
    uint64_t q;               /* documents of the last launch of either kind                          */
    uint64_t positions;       /* positions of the last score launches                                 */
    double   match_ms;        /* HIP-event time of the last three match launches together             */
    double   score_ms;        /* ... of the last three score launches together                        */
    double   docs_ms;         /* ... of the last score docs launch                                    */
} sa_hip_token_shards_score_stats;

/* merged_dev: NULL, or sa_hip_token_shards_match[total] as sa_hip_token_shards_match_batch_device wrote them for this batch and
 * max_length; scores_dev: sa_hip_token_shards_score[total]; per_shard_dev: sa_hip_token_span[S * total]; total = offsets[Q]. */
int sa_hip_token_shards_score_batch_device(sa_hip_token_shards* set, const void* patterns_dev, const void* offsets_dev, uint64_t Q,
                                           uint64_t total, uint32_t max_length, const void* merged_dev, void* scores_dev,
                                           void* per_shard_dev);
/* scores_dev as the call above writes them (may be NULL when every document is empty); heads_dev: sa_hip_token_score_head[Q]. */
int sa_hip_token_shards_score_docs_batch_device(sa_hip_token_shards* set, const void* scores_dev, const void* offsets_dev, uint64_t Q,
                                                void* heads_dev);
/* Host pointers; scores[offsets[Q]], per_shard[S * offsets[Q]] and heads[Q] out, any of them may be NULL, not all three. */
int sa_hip_token_shards_score_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    uint32_t max_length, sa_hip_token_shards_score* scores, sa_hip_token_span* per_shard,
                                    sa_hip_token_score_head* heads);
int sa_hip_token_shards_score_info(const sa_hip_token_shards* set, sa_hip_token_shards_score_stats* out);

/* (6k) top-k next symbols and draws from a span (csrc/token_top.hpp, csrc/capi_token_top.hpp): which k symbols follow a context
 * most often, and a next symbol drawn with the corpus's probability.  All results are exact.
 *
 * Spans, modes, need_next and max_length are those of (6b); start = first + ended and total = count - ended are the ranks of a
 * span that have a next symbol s(r) = T[SA[r] + length], non-decreasing in r.
 *   top     the walked ranks are [start, start + walked), walked = budget ? min(total, budget) : total.  Where (6b) gives the cap
 *           smallest symbols, this gives the k (1 .. 64) most frequent among the walked ranks: symbols[i * k ..] and
 *           counts[i * k ..] sorted by count descending, ties by symbol ascending; a symbol whose ranks the budget cuts counts
 *           with those inside.  Cells beyond heads[i].written are not written.  The answer is the true top-k of the span iff
 *           budget == 0 || total <= budget.
 *   sample  m draws per span, draws[i * m + j] any uint64: rank = start + floor(draw * total / 2^64), symbol = s(rank), to
 *           symbols[i * m + j] and (unless NULL) ranks[i * m + j]; total == 0 gives symbol -1 and rank 0xFFFFFFFF.  Nothing random
 *           happens on the device: the same draws give the same answers, and a uniform draw gives every next symbol its corpus
 *           probability count / total to within 2^-64 * total.
 *
 * Errors: a NULL handle or argument, mode or need_next other than 0 / 1, k == 0, k > 64, m == 0, Q * k or Q * m >= 2^31 and
 * descending offsets return -1 before any HIP call; Q == 0 is a no-op.  The device forms are asynchronous on the handle's stream
 * until sa_hip_token_index_sync and chain behind sa_hip_token_index_spans_batch_device without a host trip; like
 * sa_hip_token_index_next_batch_device they trust nothing: first and count are clamped to the array, and an array that is not the
 * suffix array gives unspecified entries from bounded loops.  The host forms stage through buffers of the handle. */
typedef struct sa_hip_token_top {
    uint32_t written;   /* entries written, = min(k, distinct)                                        */
    uint32_t distinct;  /* distinct next symbols among the walked ranks                               */
    uint32_t covered;   /* sum of the written counts                                                  */
    uint32_t total;     /* count - ended (as sa_hip_token_next.total); walked = budget ? min(total, budget) : total */
} sa_hip_token_top;

typedef struct sa_hip_token_top_info {
    uint64_t q;            /* spans of the last top or sample launch                            */
    double   spans_ms;     /* HIP-event time of the last span launch (the call waits for it)    */
    double   top_ms;       /* ... of the last top launch                                        */
    double   sample_ms;    /* ... of the last sample launch                                     */
} sa_hip_token_top_info;

/* spans_dev: sa_hip_token_span[Q]; symbols_dev: int32[Q * k]; counts_dev: uint32[Q * k]; heads_dev: sa_hip_token_top[Q]. */
int sa_hip_token_index_top_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, uint32_t k, uint32_t budget,
                                        void* symbols_dev, void* counts_dev, void* heads_dev);
/* Both steps from host contexts: spans (may be NULL), symbols, counts and heads out. */
int sa_hip_token_index_top_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                 int mode, uint32_t max_length, int need_next, uint32_t k, uint32_t budget,
                                 sa_hip_token_span* spans, int32_t* symbols, uint32_t* counts, sa_hip_token_top* heads);
/* draws_dev: uint64[Q * m]; symbols_dev: int32[Q * m]; ranks_dev: uint32[Q * m], may be NULL. */
int sa_hip_token_index_sample_batch_device(sa_hip_token_index* t, const void* spans_dev, uint64_t Q, const void* draws_dev,
                                           uint32_t m, void* symbols_dev, void* ranks_dev);
/* Both steps from host contexts and host draws: spans (may be NULL), symbols and ranks (may be NULL) out. */
int sa_hip_token_index_sample_batch(sa_hip_token_index* t, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                    int mode, uint32_t max_length, int need_next, const uint64_t* draws, uint32_t m,
                                    sa_hip_token_span* spans, int32_t* symbols, uint32_t* ranks);
int sa_hip_token_index_top_info(const sa_hip_token_index* t, sa_hip_token_top_info* out);

/* (6l) top-k next symbols and draws over a shard set (csrc/token_shard_top.hpp, csrc/capi_token_shard_top.hpp): the calls of (6k)
 * answered over all shards of a set.  All results are exact.  An exact top-k of counts summed over shards cannot be merged from
 * the shards' own top-k lists (a symbol that is (k+1)-th in every shard can be first overall), so one kernel walks the S spans of a
 * context side by side and sums equal symbols as it goes; it keeps no per-shard lists: no scratch budget, no chunks.
 *
 * Spans, modes, need_next, max_length and the layout spans[s * Q + i] are those of (6c).  For shard s of context i: start_s =
 * first + ended and total_s = count - ended (both after clamping to the shard's array); total = sum over s of total_s, a uint64.
 *   top     the continuations of a context are taken in the set's merged order, ascending by next symbol -- the suffix order of a
 *           single index over the whole corpus; walked = budget ? min(total, budget) : total, budget a uint64.  The k (1 .. 64)
 *           most frequent next symbols among the first `walked` continuations, their counts summed over the shards as uint64:
 *           symbols[i * k ..] (int32) and counts[i * k ..] (uint64) sorted by count descending, ties by symbol ascending.  The
 *           merged run that the budget cuts counts with what lies inside (which shard's ranks those are does not matter: only the
 *           sum is reported).  Cells beyond heads[i].written are not written.  The answer is the true top-k iff budget == 0 ||
 *           total <= budget.  With these definitions the answer equals what sa_hip_token_index_top_batch gives on one index over
 *           the uncut corpus, at every S.
 *   sample  m draws per context, draws[i * m + j] any uint64: r = floor(draw * total / 2^64).  The continuations are numbered
 *           shard-major -- shard 0's ranks [start_0, start_0 + total_0) first, then shard 1's, and so on: s is the shard with
 *           before_s <= r < before_s + total_s, rank = start_s + (r - before_s), symbol = s_s(rank) read at that shard's span
 *           length.  symbols int32[Q * m], shards_out uint32[Q * m] and ranks uint32[Q * m]; the last two may be NULL, each on
 *           its own.  total == 0 gives -1 / 0xFFFFFFFF / 0xFFFFFFFF.  Nothing random happens on the device, and a uniform draw
 *           gives every next symbol count / total, its probability over the whole corpus.  The mapping from draw to symbol is
 *           shard-major, not symbol-major: for S > 1 it differs from that of a single index over the uncut corpus (6k); the
 *           distribution is the same, and at S == 1 the mapping is identical.
 *
 * Errors: a NULL set or required pointer, mode or need_next other than 0 / 1, k == 0, k > 64, m == 0, Q * k or Q * m >= 2^31 and
 * descending offsets return -1 before any HIP call (Q * k < 2^31 and S <= 64 keep Q * S within one launch: there is no separate
 * limit); Q == 0 is a no-op.  The device forms are asynchronous on the set's stream until sa_hip_token_shards_sync and chain behind
 * sa_hip_token_shards_spans_batch_device without a host trip; they trust nothing: spans are clamped per shard, every loop is
 * bounded, and an array that is not the suffix array gives unspecified entries, never an access outside the buffers.  The host
 * forms stage through buffers of the set. */
typedef struct sa_hip_token_shards_top {
    uint32_t written;   /* entries written, = min(k, distinct)                                        */
    uint32_t distinct;  /* merged next symbols among the walked continuations                         */
    uint32_t length;    /* the largest `length` among the context's S spans (as sa_hip_token_shards_next.length) */
    uint32_t shards;    /* shards with total_s > 0                                                    */
    uint64_t covered;   /* sum of the written counts                                                  */
    uint64_t total;     /* sum over s of total_s; walked = budget ? min(total, budget) : total       */
} sa_hip_token_shards_top;

typedef struct sa_hip_token_shards_top_stats {
    uint64_t q;            /* contexts of the last top or sample launch                         */
    double   spans_ms;     /* HIP-event time of the last spans launch (the call waits for it)   */
    double   top_ms;       /* ... of the last top launch                                        */
    double   sample_ms;    /* ... of the last sample launch                                     */
} sa_hip_token_shards_top_stats;

/* spans_dev: sa_hip_token_span[S * Q]; symbols_dev: int32[Q * k]; counts_dev: uint64[Q * k]; heads_dev: sa_hip_token_shards_top[Q]. */
int sa_hip_token_shards_top_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t Q, uint32_t k, uint64_t budget,
                                         void* symbols_dev, void* counts_dev, void* heads_dev);
/* Both steps from host contexts: spans[S * Q] (may be NULL), symbols, counts and heads out. */
int sa_hip_token_shards_top_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                  int mode, uint32_t max_length, int need_next, uint32_t k, uint64_t budget,
                                  sa_hip_token_span* spans, int32_t* symbols, uint64_t* counts, sa_hip_token_shards_top* heads);
/* draws_dev: uint64[Q * m]; symbols_dev: int32[Q * m]; shards_dev and ranks_dev: uint32[Q * m], each may be NULL. */
int sa_hip_token_shards_sample_batch_device(sa_hip_token_shards* set, const void* spans_dev, uint64_t Q, const void* draws_dev,
                                            uint32_t m, void* symbols_dev, void* shards_dev, void* ranks_dev);
/* Both steps from host contexts and host draws: spans[S * Q] (may be NULL), symbols, shards_out and ranks (may be NULL) out. */
int sa_hip_token_shards_sample_batch(sa_hip_token_shards* set, const int32_t* patterns, const uint64_t* offsets, uint64_t Q,
                                     int mode, uint32_t max_length, int need_next, const uint64_t* draws, uint32_t m,
                                     sa_hip_token_span* spans, int32_t* symbols, uint32_t* shards_out, uint32_t* ranks);
int sa_hip_token_shards_top_info(const sa_hip_token_shards* set, sa_hip_token_shards_top_stats* out);

/* ---- instrumentation ---------------------------------------------------------------------- */

/* Per-build statistics of the last build on this handle (roofline accounting). */
typedef struct sa_hip_build_stats {
    uint64_t n;
    uint32_t sigma;              /* distinct byte values                                   */
    uint32_t bits_per_symbol;    /* b: code width after alphabet compaction                */
    uint32_t initial_chars;      /* K0: characters packed into the initial 64-bit key      */
    uint32_t rounds;             /* refinement rounds after the initial sort               */
    uint32_t chunk_rounds;
    uint32_t doubling_rounds;
    uint32_t final_depth;        /* h when the active set became empty                     */
    uint32_t radix_passes;       /* onesweep launches over all sorts                       */
    uint64_t radix_records;      /* sum over passes of records moved                       */
    uint64_t radix_bytes;        /* algorithmic bytes of those passes (read + written)    */
    uint64_t active_total;       /* sum over rounds of active-set sizes                    */
    uint64_t tiny_resolved;      /* suffixes ordered by the tiny-group finisher            */
    double   radix_ms;           /* HIP-event time of all onesweep launches                */
    double   total_ms;           /* HIP-event time of the whole device build               */
    /* the sort passes by kernel: [0] radix_onesweep_kernel<512> (u64 key + u32 value in and out),
     * [1] top digit of a narrow sort (u32 key + u32 value out): radix_onesweep_kernel<512,0,true> from u64
     *     keys, or text_top_pass_kernel<512> from the text (text_top_pass),
     * [2] seg_onesweep_kernel<512,24,false,true> (u32 key + u32 value in and out),
     * [3] seg_onesweep_kernel<512,24,true,true>: last narrow pass (u32 key + u32 value in; out: u32 key + u32 value when
     *     the index keeps the narrow keys (narrow_k), else rebuilt u64 key + u32 value) */
    double   pass_ms[4];
    uint64_t pass_bytes[4];      /* algorithmic bytes (read + written)                      */
    uint32_t pass_launches[4];
    uint32_t text_top_pass;      /* 1: kernel [1] was text_top_pass_kernel<512> (keys assembled from the text) */
    uint32_t narrow_k;           /* 1: the index keeps u32 narrow keys + 257 bucket bounds as its query key array   */
    double   widen_ms;           /* HIP-event time of the last sa_hip_index_widen_device after this build (0: none)  */
    uint64_t finisher_records;   /* records of groups that fit a tile, summed over the runs of the in-LDS group finisher */
    uint64_t finisher_resolved;  /* suffixes it ordered finally (they never see a global refinement round)            */
    uint32_t finisher_runs;
    uint32_t widen_fused;        /* 1: the int64 copy of sa_hip_index_build_device64 came out of the sort's last pass       */
    uint32_t narrow48;           /* 1: keys of 41..56 bits sorted as 10-byte records (u32 + u16 key parts + u32 index): kernels [1] =
                                  *    text_top_pass_kernel<512, true>, [2] / [3] = seg48_onesweep_kernel                           */
    uint32_t lite_flags;         /* 1: the first flags pass wrote no flag array (near-random text: active records staged per tile);
                                  * 2: there was no such pass at all -- the local pass of the three-pass plan did its work per sub-bucket */
    uint64_t period_resolved;    /* suffixes ordered by the periodic-run shortcut (long repeats: period_finish.hpp)              */
    uint32_t split_plan;         /* > 0 (= rb, the key bits of the split): the narrow sort ran as THREE passes over the records (radix_split.hpp): kernels [2] = seg_split_kernel
                                  *    (one launch: the records of a bucket grouped by their next rb <= 10 key bits), [3] = local_finish_kernel (one
                                  *    launch: every group ordered completely in LDS, suffixes out as u32 and, for a 64-bit build, int64)        */
    uint32_t split_max;          /* largest group at the level taken (declined: at the finest level, > 8192); 0: the plan was not considered      */
} sa_hip_build_stats;
int sa_hip_index_build_stats(const sa_hip_index* idx, sa_hip_build_stats* out);

/* Statistics of the search launches on this handle.  kernel_ms: the last launch; kernel_ms_sum / launches: every launch
 * since the previous call of sa_hip_index_query_stats (a pipelined step issues several; the library keeps HIP events
 * for the last 32 launches and resolves them here -- the call waits for them). */
typedef struct sa_hip_query_stats {
    uint64_t q;                  /* patterns of the last launch                            */
    double   kernel_ms;          /* HIP-event time of the last search kernel               */
    double   kernel_ms_sum;      /* ... of all launches since the previous call            */
    uint32_t launches;
    uint32_t pad_;
} sa_hip_query_stats;
int sa_hip_index_query_stats(const sa_hip_index* idx, sa_hip_query_stats* out);

/* ---- host-side CSV column extractor (reference engine.c:26-96, 461-654) ----------- */

/* One column of an RFC-4180 CSV file, prepared for sa_hip_index_build: the fields lower-cased (ASCII)
 * with a '\n' after each, the offset of every row's field in that text and the byte offset of every
 * row in the file (num_rows + 1 entries: the last one is the end of the last row).  The header row
 * is not indexed.  All arrays are malloc'ed by the callee; release with sa_hip_csv_free. */
typedef struct sa_hip_csv_column {
    uint8_t*  text;
    uint64_t  text_len;
    uint64_t* row_text_starts;
    uint64_t* row_file_offsets;
    uint64_t  num_rows;
    char*     column_names;      /* num_columns NUL-terminated names, back to back */
    uint32_t  num_columns;
    uint32_t  column_index;
} sa_hip_csv_column;
int sa_hip_csv_extract_column(const char* path, const char* column, sa_hip_csv_column* out);
void sa_hip_csv_free(sa_hip_csv_column* col);
/* Synthetic `id,company_name,country` CSV of BASELINE config 5. */
int sa_hip_synth_csv(const char* path, uint64_t rows, uint64_t seed);

/* Stable LSD radix sort of n (u64 key, u32 value) records by key bits [begin_bit, end_bit) on
 * `device` (host pointers, sorted in place).  The device sort underneath every build, exported
 * so that it can be tested and profiled on its own.  values == NULL: values are the record
 * positions 0..n-1 and are not returned. */
int sa_hip_sort_pairs(uint64_t* keys, uint32_t* values, uint64_t n, int begin_bit, int end_bit, int device);

/* Synthetic text D1 `uniform27` of SURVEY.md 8(d): xorshift64 stream, 26 letters + '\n'. */
void sa_hip_synth_uniform27(uint8_t* out, uint64_t n, uint64_t seed);

const char* sa_hip_last_error(void);
const char* sa_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SA_HIP_H */
