// th_pack_sidechains: a rotamer SEARCH for a batch of structures — for every residue the class, among the 3^n_chi classes of its
// type built at their bin centres, that a steric ladder and optionally a model's own probabilities prefer, found by greedy sweeps
// from a deterministic start.  th_build_sidechains (sidechains.hip) builds what the caller chose; this chooses.  The rule is written
// out in include/timed_hip.h.
//
//     *** PARITY UNPINNED AGAINST SCWRL4 ***  The reference hands sequence and backbone to SCWRL4 (analyse_rotamers.py analyses 2
//     and 3), which is not available where this project is built.  The rule is this project's own: no backbone-dependent rotamer
//     library, no SCWRL4 energy, no hydrogen bonds, no global optimum.
//
// k_pack_candidates: the 16 lanes per residue of k_build_sidechains with one "residue" per candidate (sidechain_place.h: the same
// float64 operations in the same order), into double[n_cand][10][3] and one validity byte per candidate.
// k_pack_backbone: a work item is (structure, 25 candidates); thread t < 250 owns atom t % 10 of candidate t / 10 and counts its
// ladder levels against the structure's backbone atoms, streamed through LDS in tiles of 256 slots as k_sidechain_clashes does.
// k_pack_search: ONE workgroup of 832 threads per structure runs the initial choice, all sweeps and the two evaluations.  It is
// serial over residues; within a step thread t owns (candidate t / 10, atom t % 10) of the residue, up to 81 x 10.  The current
// side-chain atoms of the structure live in global memory and are read through LDS: a structure of at most `tile` residues stays
// resident there for the whole search (every move is written to both), a longer one is streamed tile after tile in every step.
// The costs of the candidates go to LDS, every thread scans them in class order (lowest cost, lowest k on ties) and so reaches the
// same decision without a second reduction.  Every thread reaches every barrier: all loop bounds and the branches that hold a
// barrier depend on the structure and the step alone, and nothing returns inside the loops; max_sweeps bounds the run.
// Everything decided is an integer; no atomics; a structure's outputs depend on its own residues alone.  No pair is culled: every
// candidate atom meets every current atom of the structure, so the result is the all-pairs rule by construction.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "common.h"
#include "oneshot.h"
#include "sidechain_place.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kPerBlock = kBlock / kLanes;     // candidates per workgroup of k_pack_candidates
constexpr int kBbCand = 25;                    // candidates per work item of k_pack_backbone: 250 of 256 threads own an atom
constexpr int kMaxCand = TH_PACK_MAX_CANDIDATES;
constexpr int kSearch = 832;                   // threads of k_pack_search: 13 wavefronts, 81 x 10 = 810 items
constexpr int kEval = 830;                     // (residue, atom) items per round of the evaluation: whole residues only
constexpr int kResTile = 200;                  // residues of current atoms in LDS at most: 200 x 248 bytes, under 64 KB with the rest
constexpr int kXyz = kScMaxAtoms * 3;          // doubles per candidate / per residue of current atoms

struct Ladder { int n; double thr[TH_PACK_MAX_LEVELS]; double top; };
struct PackTab { int n_chi[kScTypes], class_base[kScTypes], sg_slot[kScTypes]; };

__constant__ PackTab c_pack;

__global__ void __launch_bounds__(kBlock) k_pack_candidates(const double* __restrict__ backbone, int nb, const signed char* __restrict__ res_type,
                                                            const long long* __restrict__ cand_off, const int* __restrict__ cand_res, long long n_cand,
                                                            double* __restrict__ cand_xyz, unsigned char* __restrict__ cand_ok) {
    const long long c = (long long)blockIdx.x * kPerBlock + threadIdx.x / kLanes;
    const int lane = threadIdx.x % kLanes;
    const bool live = c < n_cand;
    const long long r = live ? cand_res[c] : 0;
    const int type = live ? (int)res_type[r] : -1;
    const int ti = type >= 0 ? type : 0;
    const int n_atoms = type >= 0 ? c_tab.n[ti] : 0;
    const int j = lane - 3;
    const bool mine = j >= 0 && j < n_atoms;
    const DevRow& row = c_tab.row[ti][mine ? j : 0];
    const double nan = __builtin_nan("");
    double px = nan, py = nan, pz = nan;
    if (live && lane < 3) {
        const size_t at = ((size_t)r * nb + lane) * 3;
        px = backbone[at], py = backbone[at + 1], pz = backbone[at + 2];
    }
    double chi_k = 0.0;
    if (mine && row.k >= 0) {                                          // the bin of angle row.k in class k: the first angle varies slowest
        int index = (int)(c - cand_off[r]);
        for (int q = c_pack.n_chi[ti] - 1; q > row.k; --q) index /= 3;
        const int bin = index % 3;
        chi_k = bin == 0 ? 60.0 : bin == 1 ? 180.0 : -60.0;
    }
    sc_place_lanes(row, mine, chi_k, px, py, pz);
    const bool bad = (lane < 3 || mine) && !finite3(px, py, pz);
    const unsigned long long bad_mask = __ballot(bad);
    const int group = (threadIdx.x % warpSize) / kLanes;
    const bool built = n_atoms > 0 && ((bad_mask >> (group * kLanes)) & 0xffffull) == 0;
    if (!live) return;
    if (j >= 0 && j < kScMaxAtoms) {
        double* out = cand_xyz + ((size_t)c * kScMaxAtoms + j) * 3;
        const bool keep = built && mine;
        out[0] = keep ? px : nan;
        out[1] = keep ? py : nan;
        out[2] = keep ? pz : nan;
    }
    if (lane == 0) cand_ok[c] = built ? 1 : 0;
}

__device__ inline int levels_under(const Ladder& lad, double s) {
    int n = 0;
    for (int t = 0; t < lad.n; ++t) n += s < lad.thr[t] ? 1 : 0;
    return n;
}

__global__ void __launch_bounds__(kBlock) k_pack_backbone(const double* __restrict__ backbone, int nb, const int* __restrict__ chain_id,
                                                          const long long* __restrict__ offsets, const long long* __restrict__ cand_off,
                                                          const int* __restrict__ cand_res, const double* __restrict__ cand_xyz,
                                                          const ThTile* __restrict__ items, Ladder lad, int* __restrict__ bb_pen) {
    __shared__ double jx[kBlock], jy[kBlock], jz[kBlock];
    __shared__ int jres[kBlock], jchain[kBlock], cnt[kBlock];
    const int tid = threadIdx.x;
    const ThTile it = items[blockIdx.x];       // candidates tile * kBbCand ... of the residues offsets[range] ... of that structure
    const long long begin = offsets[it.range], end = offsets[it.range + 1];
    const int len = (int)(end - begin);
    const long long c = cand_off[begin] + (long long)it.tile * kBbCand + tid / kScMaxAtoms;
    const int slot = tid % kScMaxAtoms;
    const bool live = tid < kBbCand * kScMaxAtoms && c < cand_off[end];
    const double nan = __builtin_nan("");
    double pi[3] = {nan, nan, nan};
    int ri = -1, chain_i = 0;
    if (live) {
        const long long r = cand_res[c];
        ri = (int)(r - begin);
        for (int a = 0; a < 3; ++a) pi[a] = cand_xyz[((size_t)c * kScMaxAtoms + slot) * 3 + a];
        chain_i = chain_id ? chain_id[r] : 0;
    }
    int pen = 0;
    const long long slots = (long long)len * nb;
    for (long long j0 = 0; j0 < slots; j0 += kBlock) {
        const long long j = j0 + tid;
        double pj[3] = {nan, nan, nan};
        int rj = 0, chain_j = 0;
        if (j < slots) {
            rj = (int)(j / nb);
            const size_t r = (size_t)(begin + rj);
            for (int a = 0; a < 3; ++a) pj[a] = backbone[(r * nb + (size_t)(j % nb)) * 3 + a];
            chain_j = chain_id ? chain_id[r] : 0;
        }
        __syncthreads();                       // the previous tile is no longer read
        jx[tid] = pj[0];
        jy[tid] = pj[1];
        jz[tid] = pj[2];
        jres[tid] = rj;
        jchain[tid] = chain_j;
        __syncthreads();
        const int m = (int)(slots - j0 < kBlock ? slots - j0 : kBlock);
        for (int jj = 0; jj < m; ++jj) {
            const double dx = jx[jj] - pi[0], dy = jy[jj] - pi[1], dz = jz[jj] - pi[2];
            const double s = (dx * dx + dy * dy) + dz * dz;
            if (s < lad.top) {                 // false for a NaN: an absent atom on either side
                const int r2 = jres[jj];
                const bool neighbour = (r2 - ri == 1 || ri - r2 == 1) && jchain[jj] == chain_i;
                if (r2 != ri && !neighbour) pen += levels_under(lad, s);
            }
        }
    }
    cnt[tid] = pen;
    __syncthreads();
    if (live && slot == 0) {
        int sum = 0;
        for (int k = 0; k < kScMaxAtoms; ++k) sum += cnt[tid + k];
        bb_pen[c] = sum;
    }
}

struct SearchArgs {
    const signed char* res_type;
    const long long* offsets;
    const long long* cand_off;
    const double* cand_xyz;
    const unsigned char* cand_ok;
    const int* bb_pen;
    const int* prior;                          // [n_res][kMaxCand] or null
    double* cur_xyz;                           // [n_res][10][3]: the atoms of the current candidate, NaN without one
    int* cur_k;                                // [n_res]: the current candidate, -1 without one
    short* out_cls;
    long long *out_cost0, *out_cost1, *out_e0, *out_e1;
    int* out_search;                           // [n_struct][4]: sweeps, moves, converged, status
    int weight, max_sweeps, tile, limit;
};

struct SearchLds {
    double* xyz;                               // [tile][10][3]
    int *n, *sg;                               // [tile]: atoms of the current candidate (0 without one), its SG slot or -1
};

__device__ inline void load_tile(const SearchArgs& a, const SearchLds& lds, long long begin, int tile0, int m) {
    const int tid = threadIdx.x;
    for (int q = tid; q < m * kXyz; q += kSearch) lds.xyz[q] = a.cur_xyz[(size_t)(begin + tile0) * kXyz + q];
    for (int q = tid; q < m; q += kSearch) {
        const long long r = begin + tile0 + q;
        const int type = a.res_type[r];
        const bool have = type >= 0 && a.cur_k[r] >= 0;
        lds.n[q] = have ? c_tab.n[type] : 0;
        lds.sg[q] = have ? c_pack.sg_slot[type] : -1;
    }
}

// the ladder levels of one atom against the current side-chain atoms of every residue of the structure but `self`.  Holds barriers
// when the structure is streamed: every thread of the workgroup calls it, an idle one with a NaN atom.
__device__ inline int pen_current(const SearchArgs& a, const SearchLds& lds, const Ladder& lad, long long begin, int len, bool resident,
                                  double px, double py, double pz, bool sg_i, int self) {
    int pen = 0;
    const bool present = px == px;             // an absent atom is within nothing: its thread (often its whole wavefront) only keeps the barriers
    for (int tile0 = 0; tile0 < len; tile0 += a.tile) {
        const int m = len - tile0 < a.tile ? len - tile0 : a.tile;
        if (!resident) {
            __syncthreads();                   // the previous tile is no longer read
            load_tile(a, lds, begin, tile0, m);
            __syncthreads();
        }
        for (int jj = 0; present && jj < m; ++jj) {
            if (tile0 + jj == self) continue;
            const int n = lds.n[jj], sg = lds.sg[jj];
            const double* q = lds.xyz + jj * kXyz;
            for (int at = 0; at < n; ++at) {
                const double dx = q[3 * at] - px, dy = q[3 * at + 1] - py, dz = q[3 * at + 2] - pz;
                const double s = (dx * dx + dy * dy) + dz * dz;
                if (s < lad.top && !(sg_i && at == sg)) pen += levels_under(lad, s);
            }
        }
    }
    return pen;
}

__global__ void __launch_bounds__(kSearch) k_pack_search(SearchArgs a, Ladder lad) {
    extern __shared__ double s_dyn[];
    __shared__ int s_pen[kSearch];
    __shared__ long long s_cost[kMaxCand];
    __shared__ long long s_red[kSearch];
    const int tid = threadIdx.x;
    const long long s = blockIdx.x;
    const long long begin = a.offsets[s], end = a.offsets[s + 1];
    const double nan = __builtin_nan("");
    if (end - begin > a.limit) {               // the whole workgroup leaves, before any barrier
        for (long long r = begin + tid; r < end; r += kSearch) {
            a.out_cls[r] = -1;
            a.out_cost0[r] = a.out_cost1[r] = 0;
        }
        if (tid == 0) {
            a.out_e0[s] = a.out_e1[s] = 0;
            a.out_search[4 * s] = a.out_search[4 * s + 1] = a.out_search[4 * s + 2] = 0;
            a.out_search[4 * s + 3] = TH_PACK_TOO_LONG;
        }
        return;
    }
    const int len = (int)(end - begin);
    const bool resident = len <= a.tile;
    SearchLds lds;
    lds.xyz = s_dyn;
    lds.n = (int*)(s_dyn + (size_t)a.tile * kXyz);
    lds.sg = lds.n + a.tile;

    // the initial state: for every residue the candidate of lowest prior + weight x backbone penalty, lowest k on ties
    int can_move = 0;
    for (int r = tid; r < len; r += kSearch) {
        const long long c0 = a.cand_off[begin + r];
        const int nc = (int)(a.cand_off[begin + r + 1] - c0);
        int best = -1, valid = 0;
        long long best_cost = 0;
        for (int k = 0; k < nc; ++k) {
            if (!a.cand_ok[c0 + k]) continue;
            ++valid;
            const long long cost = (a.prior ? (long long)a.prior[(size_t)(begin + r) * kMaxCand + k] : 0) + (long long)a.weight * a.bb_pen[c0 + k];
            if (best < 0 || cost < best_cost) best = k, best_cost = cost;
        }
        a.cur_k[begin + r] = best;
        for (int q = 0; q < kXyz; ++q) a.cur_xyz[(size_t)(begin + r) * kXyz + q] = best >= 0 ? a.cand_xyz[(size_t)(c0 + best) * kXyz + q] : nan;
        can_move |= valid >= 2 ? 1 : 0;
    }
    const int movable = __syncthreads_or(can_move);
    if (resident) {
        load_tile(a, lds, begin, 0, len);
        __syncthreads();
    }

    // the cost of every residue in the current state and the structure's energy: thread t < 830 owns (residue, atom) items
    auto evaluate = [&](long long* out_cost, long long* out_energy) {
        long long twice = 0;                   // 2 x (prior + weight x backbone) + weight x (side chain penalty seen from this residue)
        for (int base = 0; base < len * kScMaxAtoms; base += kEval) {
            const int item = base + tid, r = item / kScMaxAtoms, at = item % kScMaxAtoms;
            const bool live = tid < kEval && r < len;
            const int k = live ? a.cur_k[begin + r] : -1;
            const int type = live ? (int)a.res_type[begin + r] : -1;
            double p[3] = {nan, nan, nan};
            if (k >= 0)
                for (int q = 0; q < 3; ++q) p[q] = a.cur_xyz[(size_t)(begin + r) * kXyz + 3 * at + q];
            const bool sg_i = k >= 0 && at == c_pack.sg_slot[type];
            s_pen[tid] = pen_current(a, lds, lad, begin, len, resident, p[0], p[1], p[2], sg_i, live ? r : -1);
            __syncthreads();
            if (live && at == 0) {
                long long sc = 0, fixed = 0;
                for (int q = 0; q < kScMaxAtoms; ++q) sc += s_pen[tid + q];
                if (k >= 0) {
                    const long long c = a.cand_off[begin + r] + k;
                    fixed = (a.prior ? (long long)a.prior[(size_t)(begin + r) * kMaxCand + k] : 0) + (long long)a.weight * a.bb_pen[c];
                }
                out_cost[begin + r] = fixed + (long long)a.weight * sc;
                twice += 2 * fixed + (long long)a.weight * sc;
            }
            __syncthreads();
        }
        s_red[tid] = twice;
        __syncthreads();
        if (tid == 0) {
            long long sum = 0;
            for (int q = 0; q < kSearch; ++q) sum += s_red[q];
            out_energy[s] = sum / 2;           // every side chain - side chain pair was seen from both ends
        }
        __syncthreads();
    };
    evaluate(a.out_cost0, a.out_e0);

    int sweeps = 0, moves = 0, converged = movable ? 0 : 1;
    const int cand_k = tid / kScMaxAtoms, cand_at = tid % kScMaxAtoms;
    for (int sweep = 0; movable && !converged && sweep < a.max_sweeps; ++sweep) {
        int moved = 0;
        for (int i = 0; i < len; ++i) {
            const long long c0 = a.cand_off[begin + i];
            const int nc = (int)(a.cand_off[begin + i + 1] - c0);
            if (nc < 2) continue;              // the same for every thread
            const int type = a.res_type[begin + i];
            const bool live = cand_k < nc;
            double p[3] = {nan, nan, nan};
            if (live)
                for (int q = 0; q < 3; ++q) p[q] = a.cand_xyz[(size_t)(c0 + cand_k) * kXyz + 3 * cand_at + q];
            const bool sg_i = cand_at == c_pack.sg_slot[type];
            s_pen[tid] = pen_current(a, lds, lad, begin, len, resident, p[0], p[1], p[2], sg_i, i);
            __syncthreads();
            if (live && cand_at == 0) {
                long long cost = LLONG_MAX;
                if (a.cand_ok[c0 + cand_k]) {
                    long long sc = 0;
                    for (int q = 0; q < kScMaxAtoms; ++q) sc += s_pen[tid + q];
                    cost = (a.prior ? (long long)a.prior[(size_t)(begin + i) * kMaxCand + cand_k] : 0) +
                           (long long)a.weight * (a.bb_pen[c0 + cand_k] + sc);
                }
                s_cost[cand_k] = cost;
            }
            __syncthreads();
            int best = 0;
            long long best_cost = s_cost[0];
            for (int k = 1; k < nc; ++k)
                if (s_cost[k] < best_cost) best = k, best_cost = s_cost[k];
            const int cur = a.cur_k[begin + i];
            const bool move = cur >= 0 && best_cost < s_cost[cur];
            __syncthreads();                   // everyone has read cur_k and s_cost
            if (move) {
                if (tid < kXyz) {
                    const double v = a.cand_xyz[(size_t)(c0 + best) * kXyz + tid];
                    a.cur_xyz[(size_t)(begin + i) * kXyz + tid] = v;
                    if (resident) lds.xyz[i * kXyz + tid] = v;
                }
                if (tid == 0) a.cur_k[begin + i] = best;
                ++moves;
                moved = 1;
            }
            __syncthreads();
        }
        ++sweeps;
        if (!moved) converged = 1;
    }

    evaluate(a.out_cost1, a.out_e1);
    for (int r = tid; r < len; r += kSearch) {
        const int k = a.cur_k[begin + r], type = a.res_type[begin + r];
        a.out_cls[begin + r] = (short)(k >= 0 ? c_pack.class_base[type] + k : -1);
    }
    if (tid == 0) {
        a.out_search[4 * s] = sweeps;
        a.out_search[4 * s + 1] = moves;
        a.out_search[4 * s + 2] = converged;
        a.out_search[4 * s + 3] = TH_PACK_OK;
    }
}

int pow3(int n) { int v = 1; while (n-- > 0) v *= 3; return v; }

}  // namespace

extern "C" int th_pack_sidechains(int device, const double* backbone, const int8_t* res_type, const int32_t* chain_id, const int64_t* struct_offsets,
                                  int64_t n_struct, int64_t n_res, const double* ladder, int n_levels, const int32_t* prior_cost,
                                  int32_t clash_weight, int32_t max_sweeps, int flags, int16_t* out_cls, int64_t* out_cost_initial,
                                  int64_t* out_cost_final, int64_t* out_energy_initial, int64_t* out_energy_final, int32_t* out_search,
                                  double* kernel_ms) {
    if (n_struct < 0 || n_res < 0)
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: negative size (n_struct = %lld, n_res = %lld)", (long long)n_struct, (long long)n_res);
    if (n_res > TH_PACK_MAX_RESIDUES || n_struct > INT_MAX)
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: %lld residues / %lld structures in one call (limits %d, 2^31 - 1)", (long long)n_res,
                (long long)n_struct, TH_PACK_MAX_RESIDUES);
    if (flags & ~TH_SC_BACKBONE_O) TH_FAIL(TH_EINVAL, "th_pack_sidechains: flags = %d has bits beyond TH_SC_BACKBONE_O", flags);
    if (n_levels < 1 || n_levels > TH_PACK_MAX_LEVELS || !ladder)
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: the ladder needs 1..%d levels, n_levels = %d", TH_PACK_MAX_LEVELS, n_levels);
    for (int t = 0; t < n_levels; ++t)
        if (!std::isfinite(ladder[t]) || ladder[t] <= 0.0 || (t > 0 && !(ladder[t] > ladder[t - 1])))
            TH_FAIL(TH_EINVAL, "th_pack_sidechains: ladder[%d] = %g: the levels are finite, positive and strictly increasing", t, ladder[t]);
    if (clash_weight < 1 || clash_weight > TH_PACK_MAX_COST)
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: clash_weight = %d outside 1..%d", (int)clash_weight, TH_PACK_MAX_COST);
    if (max_sweeps < 0 || max_sweeps > TH_PACK_MAX_SWEEPS)
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: max_sweeps = %d outside 0..%d", (int)max_sweeps, TH_PACK_MAX_SWEEPS);
    if (kernel_ms) std::memset(kernel_ms, 0, 3 * sizeof(double));
    if (n_struct == 0 && n_res != 0) TH_FAIL(TH_EINVAL, "th_pack_sidechains: n_struct = 0 owns no residue, n_res = %lld", (long long)n_res);
    if (n_struct == 0) return TH_OK;
    if (!struct_offsets) TH_FAIL(TH_EINVAL, "th_pack_sidechains: n_struct = %lld needs struct_offsets", (long long)n_struct);
    if (int rc = th_check_offsets("th_pack_sidechains", "struct_offsets", "n_res", struct_offsets, n_struct, n_res)) return rc;
    if (!out_energy_initial || !out_energy_final || !out_search)
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: n_struct = %lld needs out_energy_initial, out_energy_final and out_search", (long long)n_struct);
    if (n_res > 0 && (!backbone || !res_type || !out_cls || !out_cost_initial || !out_cost_final))
        TH_FAIL(TH_EINVAL, "th_pack_sidechains: n_res = %lld needs backbone, res_type, out_cls, out_cost_initial and out_cost_final", (long long)n_res);
    PackTab tab;
    for (int t = 0; t < kScTypes; ++t) {
        if (th_rotamer_table(t, &tab.n_chi[t], &tab.class_base[t], nullptr) != TH_OK) return TH_EINVAL;
        tab.sg_slot[t] = -1;
        for (int j = 0; j < kSidechains[t].n; ++j)
            if (pack_name(kSidechains[t].row[j].name) == host_table().sg) tab.sg_slot[t] = j;
    }
    for (int64_t r = 0; r < n_res; ++r) {
        if (res_type[r] < -1 || res_type[r] >= kScTypes)
            TH_FAIL(TH_EINVAL, "th_pack_sidechains: res_type[%lld] = %d outside -1..%d", (long long)r, (int)res_type[r], kScTypes - 1);
        if (prior_cost && res_type[r] >= 0 && kSidechains[res_type[r]].n > 0) {
            const int nc = pow3(tab.n_chi[res_type[r]]);
            for (int k = 0; k < nc; ++k) {
                const int32_t v = prior_cost[(size_t)r * kMaxCand + k];
                if (v < 0 || v > TH_PACK_MAX_COST)
                    TH_FAIL(TH_EINVAL, "th_pack_sidechains: prior_cost[%lld][%d] = %d outside 0..%d", (long long)r, k, (int)v, TH_PACK_MAX_COST);
            }
        }
    }
    const int nb = (flags & TH_SC_BACKBONE_O) ? 4 : 3;
    const size_t nr = (size_t)n_res, ns = (size_t)n_struct;
    // the candidates: 3^n_chi per residue that has a side chain and a finite N, CA, C, in a structure within the limit
    std::vector<long long> cand_off;
    std::vector<int> cand_res;
    std::vector<ThTile> items;
    int max_len = 0;
    try {
        cand_off.assign(nr + 1, 0);
        for (int64_t s = 0; s < n_struct; ++s) {
            const int64_t lo = struct_offsets[s], hi = struct_offsets[s + 1];
            const bool packed = hi - lo <= TH_PACK_MAX_STRUCT_RESIDUES;
            if (packed && hi - lo > max_len) max_len = (int)(hi - lo);
            for (int64_t r = lo; r < hi; ++r) {
                int nc = 0;
                const int type = res_type[r];
                if (packed && type >= 0 && kSidechains[type].n > 0) {
                    bool finite = true;
                    for (int q = 0; q < 9; ++q) finite = finite && std::isfinite(backbone[(size_t)r * nb * 3 + q]);
                    if (finite) nc = pow3(tab.n_chi[type]);
                }
                cand_off[r + 1] = cand_off[r] + nc;
                for (int k = 0; k < nc; ++k) cand_res.push_back((int)r);
            }
            const int64_t tiles = (cand_off[hi] - cand_off[lo] + kBbCand - 1) / kBbCand;
            for (int64_t t = 0; t < tiles; ++t) items.push_back(ThTile{(int)s, (int)t});
        }
    } catch (const std::bad_alloc&) {
        TH_FAIL(TH_ENOMEM, "th_pack_sidechains: out of host memory for the candidates of %lld residues", (long long)n_res);
    }
    const size_t ncand = cand_res.size();
    Ladder lad;
    std::memset(&lad, 0, sizeof lad);
    lad.n = n_levels;
    for (int t = 0; t < n_levels; ++t) lad.thr[t] = th_packing_threshold(ladder[t]);
    lad.top = lad.thr[n_levels - 1];
    const int tile = max_len < 1 ? 1 : max_len < kResTile ? max_len : kResTile;
    const size_t lds_bytes = (size_t)tile * (kXyz * sizeof(double) + 2 * sizeof(int));

    ThLayout lay;
    const size_t o_bb = lay.take(nr * nb * 3 * sizeof(double)), o_type = lay.take(nr), o_chain = lay.take(chain_id ? nr * sizeof(int32_t) : 0);
    const size_t o_soff = lay.take((ns + 1) * sizeof(int64_t)), o_coff = lay.take((nr + 1) * sizeof(long long)), o_cres = lay.take(ncand * sizeof(int));
    const size_t o_cxyz = lay.take(ncand * kXyz * sizeof(double)), o_cok = lay.take(ncand), o_bbpen = lay.take(ncand * sizeof(int));
    const size_t o_prior = lay.take(prior_cost ? nr * kMaxCand * sizeof(int32_t) : 0), o_items = lay.take(items.size() * sizeof(ThTile));
    const size_t o_cur = lay.take(nr * kXyz * sizeof(double)), o_curk = lay.take(nr * sizeof(int)), o_cls = lay.take(nr * sizeof(int16_t));
    const size_t o_c0 = lay.take(nr * sizeof(int64_t)), o_c1 = lay.take(nr * sizeof(int64_t)), o_e0 = lay.take(ns * sizeof(int64_t));
    const size_t o_e1 = lay.take(ns * sizeof(int64_t)), o_search = lay.take(ns * 4 * sizeof(int32_t));
    ThCall call;
    if (int rc = call.open("th_pack_sidechains", device, lay.bytes, kernel_ms ? 4 : 0)) return rc;
    double *d_bb = call.at<double>(o_bb), *d_cxyz = call.at<double>(o_cxyz);
    signed char* d_type = call.at<signed char>(o_type);
    int* d_chain = chain_id ? call.at<int>(o_chain) : nullptr;
    long long *d_soff = call.at<long long>(o_soff), *d_coff = call.at<long long>(o_coff);
    int *d_cres = call.at<int>(o_cres), *d_bbpen = call.at<int>(o_bbpen);
    unsigned char* d_cok = call.at<unsigned char>(o_cok);
    int* d_prior = prior_cost ? call.at<int>(o_prior) : nullptr;
    ThTile* d_items = call.at<ThTile>(o_items);
    hipStream_t st = call.st[0];
    const DevTable& dev_tab = host_table();
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_tab), &dev_tab, sizeof dev_tab, 0, hipMemcpyHostToDevice, st));   // the same bytes every call
    HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(c_pack), &tab, sizeof tab, 0, hipMemcpyHostToDevice, st));
    if (nr) {
        HIP_TRY(hipMemcpyAsync(d_bb, backbone, nr * nb * 3 * sizeof(double), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_type, res_type, nr, hipMemcpyHostToDevice, st));
        if (d_chain) HIP_TRY(hipMemcpyAsync(d_chain, chain_id, nr * sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (d_prior) HIP_TRY(hipMemcpyAsync(d_prior, prior_cost, nr * kMaxCand * sizeof(int32_t), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipMemcpyAsync(d_soff, struct_offsets, (ns + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_coff, cand_off.data(), (nr + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    if (ncand) HIP_TRY(hipMemcpyAsync(d_cres, cand_res.data(), ncand * sizeof(int), hipMemcpyHostToDevice, st));
    if (!items.empty()) HIP_TRY(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(ThTile), hipMemcpyHostToDevice, st));
    HIP_TRY(call.mark(0));
    if (ncand) {
        hipLaunchKernelGGL(k_pack_candidates, dim3((unsigned)((ncand + kPerBlock - 1) / kPerBlock)), dim3(kBlock), 0, st, d_bb, nb, d_type, d_coff, d_cres,
                           (long long)ncand, d_cxyz, d_cok);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(1));
    if (!items.empty()) {
        hipLaunchKernelGGL(k_pack_backbone, dim3((unsigned)items.size()), dim3(kBlock), 0, st, d_bb, nb, d_chain, d_soff, d_coff, d_cres, d_cxyz, d_items,
                           lad, d_bbpen);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(call.mark(2));
    SearchArgs a;
    a.res_type = d_type, a.offsets = d_soff, a.cand_off = d_coff, a.cand_xyz = d_cxyz, a.cand_ok = d_cok, a.bb_pen = d_bbpen, a.prior = d_prior;
    a.cur_xyz = call.at<double>(o_cur), a.cur_k = call.at<int>(o_curk), a.out_cls = call.at<short>(o_cls);
    a.out_cost0 = call.at<long long>(o_c0), a.out_cost1 = call.at<long long>(o_c1);
    a.out_e0 = call.at<long long>(o_e0), a.out_e1 = call.at<long long>(o_e1), a.out_search = call.at<int>(o_search);
    a.weight = clash_weight, a.max_sweeps = max_sweeps, a.tile = tile, a.limit = TH_PACK_MAX_STRUCT_RESIDUES;
    hipLaunchKernelGGL(k_pack_search, dim3((unsigned)ns), dim3(kSearch), lds_bytes, st, a, lad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(call.mark(3));
    if (nr) {
        HIP_TRY(hipMemcpyAsync(out_cls, a.out_cls, nr * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_cost_initial, a.out_cost0, nr * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_cost_final, a.out_cost1, nr * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_energy_initial, a.out_e0, ns * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_energy_final, a.out_e1, ns * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out_search, a.out_search, ns * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    return call.finish(kernel_ms, 3);
}
