// Where things lie in the buffers that the stages of a fused screen call (api_lloyd_fused.inc) and its kernels share: the
// table of record.  Plain C++17, included by host and device code alike.  Inside kernels these are constants and constexpr
// offset arithmetic only -- no pointer-returning accessors, no views: those change the code the compiler makes.
#pragma once
#include <cstddef>

// ---- the call's counters, ctx->nlist (unsigned words; `counters` / `nlist` in the kernels) --------------------------------
// Words [0, NL_PER_CALL_END) belong to one call and are zeroed at its top, but for the running total that lies among them;
// everything from NL_PER_CALL_END on is a running total over the context (or is overwritten by every call: NL_SCREENED)
// and is zeroed once, when the buffer is made.  The first SPKM_REPORT_WORDS words go to the host policy (k_call_tail).
enum spkm_counter_slot : int {
    NL_LISTED = 0,         // points the certificate could not settle: the length of list[] (k_combine_screen)
    NL_AMBIG = 1,          // points whose runner-up is within 2.25x of the winner
    NL_EARLY = 2,          // (step, tile) pairs the hinted screen finished early (k_screen_quad)
    NL_SKIPPED = 3,        // 16-point steps settled by the carried bounds
    NL_TODO = 4,           // length of todo[]: the steps / points the bounds test listed (k_bounds_steps)
    NL_CHANGED = 5,        // "some assignment changed": the gate of the counting-sort reuse
    NL_MSTEPS = 6,         // 16-point steps that only the movers unsettle: test B passed, test A did not (k_bounds_steps)
    NL_TODO_M = 7,         // length of todo_m[]: those steps, listed for the mover tile (0 with the form off)
    NL_SKIPPED_TOTAL = 8,  // u64, running: steps skipped
    NL_MCERT = 10,         // steps certified on the mover tile (k_certify_movers) ...
    NL_MSENT = 11,         // ... and steps it sent on to todo[] instead
    NL_KEPT = 12,          // points that passed the carried-bounds test
    NL_EXACT_PTS = 13,     // points the exact pass processes (k_cluster_need)
    NL_MOVERS = 14,        // points that changed cluster
    NL_EVENTS = 16,        // events recorded (or only counted, past the cap)
    NL_GATE_EVENTS = 18,   // k_pick_form opened the events ...
    NL_GATE_FULL = 19,     // ... or the full pass
    NL_CHECK_DIFF = 20,    // places where d_assign differs from the library's copy (count_assign_diff)
    NL_ONE_CLUSTER = 21,   // 16-point steps whose points share one cluster
    NL_MEARLY = 22,        // steps the hinted mover launch finished early (NL_EARLY stays the main launch's)
    NL_MSTEPS2 = 23,       // steps that only the SPKM_MOVERS2 largest movers unsettle: test B2 passed, test B did not (k_bounds_steps)
    NL_TODO_M2 = 24,       // length of todo_m2[]: those steps, listed for the two mover tiles (0 with the second level off)
    NL_MCERT2 = 25,        // steps certified on the two mover tiles (k_certify_movers<2>) ...
    NL_MSENT2 = 26,        // ... and steps it sent on to todo[] instead
    NL_MEARLY2 = 27,       // (step, tile) pairs the hinted launch over todo_m2[] finished early (moved here from NL_EARLY by k_certify_movers<2>)
    NL_PER_CALL_END = 32,
    NL_EXACT_TOTAL = 32,    // u64, running: points the exact passes processed
    NL_ROUNDS_DONE = 34,    // u64, running: screen rounds executed for all centroids of a tile
    NL_ROUNDS_FULL = 36,    // u64, running: rounds of launches that do all the work
    NL_SCREENED_TOTAL = 38, // u64, running: points screened
    NL_SCREENED = 40,       // points this call screened (written by every call's tail, never zeroed)
    NL_WORDS = 64           // the buffer
};
constexpr int SPKM_REPORT_WORDS = 28;     // counters a fused call reports to the host, followed by the report's number ...
constexpr int SPKM_REPORT_BUF_WORDS = 32; // ... in this much pinned host memory (spkm_shard::h_nlist)
// the two ranges zeroed at the top of a call: the per-call words on either side of NL_SKIPPED_TOTAL
constexpr int NL_ZERO_A = 0, NL_ZERO_A_END = NL_SKIPPED_TOTAL;
constexpr int NL_ZERO_B = NL_SKIPPED_TOTAL + 2, NL_ZERO_B_END = NL_PER_CALL_END;

constexpr bool nl_zeroed(int w) { return (w >= NL_ZERO_A && w < NL_ZERO_A_END) || (w >= NL_ZERO_B && w < NL_ZERO_B_END); }
constexpr bool nl_reported(int w) { return w < SPKM_REPORT_WORDS; }
constexpr bool nl_total_ok(int w) { return w % 2 == 0 && w + 1 < NL_WORDS && !nl_zeroed(w) && !nl_zeroed(w + 1); }
static_assert(nl_reported(NL_LISTED) && nl_reported(NL_AMBIG) && nl_reported(NL_EARLY) && nl_reported(NL_SKIPPED) &&
              nl_reported(NL_KEPT) && nl_reported(NL_MOVERS) && nl_reported(NL_GATE_FULL) && nl_reported(NL_ONE_CLUSTER),
              "every counter the host policy reads is in the report");
static_assert(SPKM_REPORT_WORDS + 1 <= SPKM_REPORT_BUF_WORDS && SPKM_REPORT_WORDS <= NL_WORDS, "the report and its number fit");
static_assert(NL_SCREENED < NL_WORDS && NL_ONE_CLUSTER < NL_PER_CALL_END, "every slot fits the buffer");
static_assert(nl_reported(NL_MSTEPS) && nl_reported(NL_MCERT) && nl_reported(NL_MSENT) && nl_zeroed(NL_MSTEPS) && nl_zeroed(NL_TODO_M) &&
              nl_zeroed(NL_MCERT) && nl_zeroed(NL_MSENT) && nl_zeroed(NL_MEARLY) && NL_MEARLY < SPKM_REPORT_WORDS,
              "the mover tile's counters are per-call words of the report");
static_assert(nl_reported(NL_MSTEPS2) && nl_reported(NL_MCERT2) && nl_reported(NL_MSENT2) && nl_reported(NL_MEARLY2) && nl_zeroed(NL_MSTEPS2) &&
              nl_zeroed(NL_TODO_M2) && nl_zeroed(NL_MCERT2) && nl_zeroed(NL_MSENT2) && nl_zeroed(NL_MEARLY2),
              "... and so are the second level's");
static_assert(nl_total_ok(NL_SKIPPED_TOTAL) && nl_total_ok(NL_EXACT_TOTAL) && nl_total_ok(NL_ROUNDS_DONE) &&
              nl_total_ok(NL_ROUNDS_FULL) && nl_total_ok(NL_SCREENED_TOTAL),
              "a running total is an aligned 64-bit pair that the per-call zeroing leaves alone");
static_assert(!nl_zeroed(NL_SCREENED) && nl_zeroed(NL_EXACT_PTS) && nl_zeroed(NL_GATE_FULL), "per-call words are zeroed, NL_SCREENED is not");

// ---- per-workgroup statistics ----------------------------------------------------------------------------------------------
// ctx->wgstat: WG_STRIDE words per workgroup of k_combine_screen, added up by k_assign_list's last workgroup
enum { WG_AMBIG = 0, WG_CHANGED = 1, WG_MOVERS = 2, WG_ONE_CLUSTER = 3, WG_STRIDE = 4 };
// ctx->bstat: BS_STRIDE words per workgroup of k_bounds_steps, added up by k_call_tail
enum { BS_KEPT = 0, BS_SKIPPED = 1, BS_STRIDE = 2 };
// ctx->nitems: the work-list lengths that the plan kernels write (ints)
enum { NI_FULL = 0, NI_EVENTS = 1, NI_PAIR_CHUNKS = 2, NI_REGROUP = 4, NI_WORDS = 16 };
// NI_EVENTS: a dual call's events (its full pass keeps NI_FULL); NI_PAIR_CHUNKS: the first level of the pair events' sort

// ---- bounds carried between screen calls, spkm_shard::hb (floats; `bnd` in the kernels) ------------------------------------
//   ub[npad] | lb[npad] | assignment[npad] (int32) | delta[K] | dmax | ... | hterm[K] at HB_HTERM | ... | movers at HB_MOVERS
//   delta[k], dmax   drift of every centroid on a point's support (k_center_drift) and its maximum
//   hterm[k]         hint_w x (full 2-norm drift)^2 per centroid: the hints' estimate, not a bound
//   movers           the SPKM_MOVERS2 centroids of largest drift, picked by k_center_drift's last workgroup (K <= SPKM_MOVER_KMAX):
//                    ticket (unsigned) | d_R, d_R2 = the largest drift among the centroids outside the first SPKM_MOVERS /
//                    outside all SPKM_MOVERS2 (two floats) | ... | list[SPKM_MOVERS2] (int, by rank: the first SPKM_MOVERS
//                    are the first level's M) | slot[K] (int: a centroid's place in the list, -1: not among them)
constexpr int HB_KMAX = 65536;           // the largest K a fused call takes
constexpr int HB_HTERM = HB_KMAX + 16;   // within the tail
constexpr int SPKM_MOVERS = 32;          // centroids on the mover tile: one full tile of the 4-lanes-per-point screen
constexpr int SPKM_MOVERS2 = 64;         // ... and on the second level's two tiles (policy.h, spkm_plan_movers2)
constexpr int SPKM_MOVER_KMIN = 64, SPKM_MOVER_KMAX = 1024; // (policy.h, spkm_plan_movers)
constexpr int SPKM_MOVER2_KMIN = 96;                        // (policy.h, spkm_plan_movers2)
constexpr int HB_MOVERS = 2 * HB_KMAX + 32;                 // behind hterm
constexpr int HB_MTICKET = HB_MOVERS, HB_MDR = HB_MOVERS + 1, HB_MLIST = HB_MOVERS + 16, HB_MDR2 = HB_MDR + 1, HB_MSLOT = HB_MLIST + SPKM_MOVERS2;
constexpr int HB_TAIL = HB_MSLOT + SPKM_MOVER_KMAX + 16; // floats behind the three per-point arrays
static_assert(HB_HTERM + HB_KMAX <= HB_MOVERS && HB_MLIST % 4 == 0, "the movers lie behind hterm[], the list 16-byte aligned");
static_assert(HB_MDR2 < HB_MLIST && HB_MLIST + SPKM_MOVERS2 <= HB_MSLOT && SPKM_MOVERS2 == 2 * SPKM_MOVERS,
              "both drifts lie in front of the list, the list of two tiles in front of the slots");
constexpr long long hb_lb(long long npad) { return npad; }
constexpr long long hb_assign(long long npad) { return 2 * npad; }
constexpr long long hb_delta(long long npad) { return 3 * npad; }
constexpr long long hb_dmax(long long npad, int K) { return 3 * npad + K; }
constexpr long long hb_hterm(long long npad) { return 3 * npad + HB_HTERM; }
constexpr long long hb_mticket(long long npad) { return 3 * npad + HB_MTICKET; }
constexpr long long hb_mdr(long long npad) { return 3 * npad + HB_MDR; }
constexpr long long hb_mdr2(long long npad) { return 3 * npad + HB_MDR2; }
constexpr long long hb_mlist(long long npad) { return 3 * npad + HB_MLIST; }
constexpr long long hb_mslot(long long npad) { return 3 * npad + HB_MSLOT; }
constexpr size_t hb_floats(long long npad) { return (size_t)3 * npad + HB_TAIL; }

// ---- block summaries of the carried bounds, spkm_shard::sp (bytes): per 1024 points the clusters present (K <= 128 bits),
// the smallest slack between the bounds, a valid flag -- mask[4 nblk] (unsigned) | slack[nblk] (float) | valid[nblk] (int)
constexpr int SP_MASK_WORDS = 4;
constexpr size_t sp_off_slack(size_t nblk) { return nblk * SP_MASK_WORDS * 4; }
constexpr size_t sp_off_valid(size_t nblk) { return nblk * (SP_MASK_WORDS * 4 + 4); }
constexpr size_t sp_bytes(size_t nblk) { return nblk * (SP_MASK_WORDS * 4 + 8); }

// ---- per-cluster cache of the unchanged-cluster shortcut, spkm_shard::cl_cache (doubles; pk = p K) --------------------------
//   LOCAL sums[pk] | counts[pk] | obj2[K] | largest distance[K] | its index[K] (long long)
constexpr size_t cc_counts(size_t pk) { return pk; }
constexpr size_t cc_obj(size_t pk) { return 2 * pk; }
constexpr size_t cc_max(size_t pk, size_t K) { return 2 * pk + K; }
constexpr size_t cc_imax(size_t pk, size_t K) { return 2 * pk + 2 * K; }
constexpr size_t cc_doubles(size_t pk, size_t K) { return 2 * pk + 3 * K; }
// ... and its flags, spkm_shard::cl_flags: CL_ROWS rows of K ints
enum { CL_NEED = 0, CL_TOUCHED = 1, CL_SAME = 2, CL_IBEG = 3, CL_ICNT = 4, CL_ROWS = 5 };
