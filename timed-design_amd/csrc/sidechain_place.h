// The device copy of the side-chain table (sidechain_table.h) and the placement arithmetic of th_build_sidechains, shared by
// sidechains.hip (k_build_sidechains: one group of 16 lanes per residue) and pack_sidechains.hip (k_pack_candidates: one group per
// rotamer candidate), so that a candidate of the packer and the atoms th_build_sidechains later builds from the chosen class are
// the same float64 operations in the same order.  Every unit that includes this keeps its own copy of c_tab in constant memory and
// uploads host_table() to it before its kernels run.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "device_math.h"
#include "sidechain_table.h"

// every float64 product and sum below is rounded separately, as the NumPy restatement's are
#pragma clang fp contract(off)

namespace {

constexpr int kLanes = 16;                     // lanes per residue: 3 backbone atoms + at most 10 side-chain atoms
constexpr double kRad = 0.017453292519943295;  // pi / 180

uint32_t pack_name(const char* s) {            // four ASCII bytes, left-justified, zero-padded, little-endian (as rotamers.hip)
    uint32_t v = 0;
    for (int i = 0; i < 4 && s[i]; ++i) v |= (uint32_t)(unsigned char)s[i] << (8 * i);
    return v;
}

struct DevRow { double x, ls, offset; uint32_t name; signed char a, b, c, k, depth, pad[3]; };
struct DevTable { int n[kScTypes]; int depth; uint32_t sg; DevRow row[kScTypes][kScMaxAtoms]; };

__constant__ DevTable c_tab;

const DevTable& host_table() {
    static const DevTable tab = [] {
        DevTable t;
        std::memset(&t, 0, sizeof t);
        t.sg = pack_name("SG");
        for (int r = 0; r < kScTypes; ++r) {
            const ScType& sc = kSidechains[r];
            t.n[r] = sc.n;
            int depth[3 + kScMaxAtoms] = {0, 0, 0};
            for (int j = 0; j < sc.n; ++j) {
                const ScRow& in = sc.row[j];
                DevRow& out = t.row[r][j];
                const double theta = in.angle * kRad;
                out.x = -(in.length * std::cos(theta));
                out.ls = in.length * std::sin(theta);
                out.offset = in.offset;
                out.name = pack_name(in.name);
                out.a = in.a, out.b = in.b, out.c = in.c, out.k = in.k;
                int d = depth[in.a] > depth[in.b] ? depth[in.a] : depth[in.b];
                d = (d > depth[in.c] ? d : depth[in.c]) + 1;
                depth[3 + j] = out.depth = (signed char)d;
                if (d > t.depth) t.depth = d;
            }
        }
        return t;
    }();
    return tab;
}

// One group of kLanes lanes places one residue.  On entry lanes 0..2 hold N, CA, C in (px, py, pz) and every other lane NaN; `mine`
// says that this lane (3 + j) owns atom j of the type, `row` is that atom's row (any row that exists otherwise) and `chi_k` the
// angle chi[row.k] in degrees (read only where row.k >= 0).  Every lane of the group must call: a loop over the tree's depth in
// which every lane fetches its three parents by shuffle and the lanes of the level place their atom.
__device__ inline void sc_place_lanes(const DevRow& row, bool mine, double chi_k, double& px, double& py, double& pz) {
    const double nan = __builtin_nan("");
    double y = nan, z = nan;
    const int pa = mine ? row.a : 0, pb = mine ? row.b : 0, pc = mine ? row.c : 0, depth = mine ? row.depth : 0;
    if (mine) {
        const double phi = ((row.k >= 0 ? chi_k : 0.0) + row.offset) * kRad;
        y = row.ls * cos(phi);
        z = row.ls * sin(phi);
    }
    const int levels = c_tab.depth;
    for (int level = 1; level <= levels; ++level) {                    // every lane shuffles, the lanes of this level place their atom
        const double ax = __shfl(px, pa, kLanes), ay = __shfl(py, pa, kLanes), az = __shfl(pz, pa, kLanes);
        const double bx = __shfl(px, pb, kLanes), by = __shfl(py, pb, kLanes), bz = __shfl(pz, pb, kLanes);
        const double cx = __shfl(px, pc, kLanes), cy = __shfl(py, pc, kLanes), cz = __shfl(pz, pc, kLanes);
        if (depth == level) {
            double ux = cx - bx, uy = cy - by, uz = cz - bz;
            const double ul = sqrt((ux * ux + uy * uy) + uz * uz);
            ux = ux / ul, uy = uy / ul, uz = uz / ul;
            const double vx = bx - ax, vy = by - ay, vz = bz - az;
            double nx = vy * uz - vz * uy, ny = vz * ux - vx * uz, nz = vx * uy - vy * ux;
            const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
            nx = nx / nl, ny = ny / nl, nz = nz / nl;
            const double mx = ny * uz - nz * uy, my = nz * ux - nx * uz, mz = nx * uy - ny * ux;
            px = cx + ((row.x * ux + y * mx) + z * nx);
            py = cy + ((row.x * uy + y * my) + z * ny);
            pz = cz + ((row.x * uz + y * mz) + z * nz);
        }
    }
}

}  // namespace
