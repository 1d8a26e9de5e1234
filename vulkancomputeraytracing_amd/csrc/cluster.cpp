// cluster.cpp -- k-d grouping of spheres into fours + conservative group boxes (cluster.hpp).
#include "cluster.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace vcrt {
namespace {

// Smallest float >= x (x finite, double).
float round_up(double x) {
    float f = static_cast<float>(x);
    if (static_cast<double>(f) < x) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    return f;
}

using Group = std::array<int32_t, 4>;

// Median splits on the widest centre axis. The left part gets ceil(groups / 2) groups rounded
// up to a multiple of 64 (more than 64 groups) or 8 (more than 8), so every subtree starts on a
// node (8 groups) and chunk (64 groups) boundary and nodes are whole subtrees; only the last
// leaf is partial.
void split(std::vector<int32_t>& idx, size_t lo, size_t hi, const vcrt_sphere* s,
           std::vector<Group>& groups) {
    const size_t n = hi - lo;
    if (n <= 4) {
        Group g{-1, -1, -1, -1};
        for (size_t k = 0; k < n; k++) g[k] = idx[lo + k];
        groups.push_back(g);
        return;
    }
    double mn[3], mx[3];
    for (int a = 0; a < 3; a++) {
        mn[a] = std::numeric_limits<double>::infinity();
        mx[a] = -mn[a];
    }
    for (size_t k = lo; k < hi; k++)
        for (int a = 0; a < 3; a++) {
            mn[a] = std::min(mn[a], static_cast<double>(s[idx[k]].center[a]));
            mx[a] = std::max(mx[a], static_cast<double>(s[idx[k]].center[a]));
        }
    int axis = 0;
    for (int a = 1; a < 3; a++)
        if (mx[a] - mn[a] > mx[axis] - mn[axis]) axis = a;
    const size_t ng = (n + 3) / 4;
    const size_t align = ng > 64 ? 64 : ng > 8 ? 8 : 1;
    const size_t left = ((ng + 1) / 2 + align - 1) / align * align;
    const size_t mid = lo + 4 * left;
    std::nth_element(idx.begin() + lo, idx.begin() + mid, idx.begin() + hi,
                     [&](int32_t x, int32_t y) {
                         const float cx = s[x].center[axis], cy = s[y].center[axis];
                         return cx < cy || (cx == cy && x < y);
                     });
    split(idx, lo, mid, s, groups);
    split(idx, mid, hi, s, groups);
}

constexpr double kU = 0x1p-24;  // fp32 unit roundoff

// Smallest float <= x (x finite, double).
float round_down(double x) {
    float f = static_cast<float>(x);
    if (static_cast<double>(f) > x) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
    return f;
}

struct Box {
    float lo[3] = {1e20f, 1e20f, 1e20f};  // padding: a point far away (its groups are empty)
    float hi[3] = {1e20f, 1e20f, 1e20f};
    float K = 0.0f;                       // margin factor 8.1u / r_min of the members
};

// Axis-aligned box of `members` (centre -+ |radius|, rounded outwards to fp32) and its margin
// factor K = 8.1u / r_min (1 + 1e-5), rounded up (inf for a zero radius: never ruled out).
Box box_of(const vcrt_sphere* s, const std::vector<int32_t>& members) {
    Box b;
    if (members.empty()) return b;
    double rmin = std::numeric_limits<double>::infinity();
    for (int32_t j : members) rmin = std::min(rmin, std::fabs(static_cast<double>(s[j].radius)));
    b.K = rmin > 0.0 ? round_up(std::min(8.1 * kU / rmin * (1.0 + 1e-5), 1e38))
                     : std::numeric_limits<float>::infinity();
    for (int a = 0; a < 3; a++) {
        double lo = std::numeric_limits<double>::infinity(), hi = -lo;
        for (int32_t j : members) {
            const double r = std::fabs(static_cast<double>(s[j].radius));
            lo = std::min(lo, s[j].center[a] - r);
            hi = std::max(hi, s[j].center[a] + r);
        }
        b.lo[a] = round_down(lo);
        b.hi[a] = round_up(hi);
    }
    return b;
}

// Element i of a pair-SoA box table (TraceParams.cbound / cnode / ctop):
//   (lox0,lox1,loy0,loy1) (loz0,loz1,hix0,hix1) (hiy0,hiy1,hiz0,hiz1) (K0,K1,0,0)
void put_box(std::vector<float>& table, size_t i, const Box& b) {
    float* t = &table[(i / 2) * 16];
    const int e = i % 2;
    t[0 + e] = b.lo[0];
    t[2 + e] = b.lo[1];
    t[4 + e] = b.lo[2];
    t[6 + e] = b.hi[0];
    t[8 + e] = b.hi[1];
    t[10 + e] = b.hi[2];
    t[12 + e] = b.K;
}

// floats in order: key(x) rises with x (-inf .. +inf, -0 below +0)
int64_t float_key(float x) {
    uint32_t b;
    std::memcpy(&b, &x, sizeof b);
    return (b & 0x80000000u) ? static_cast<int64_t>(0x7fffffffu) - static_cast<int64_t>(b & 0x7fffffffu)
                             : static_cast<int64_t>(0x80000000u) + static_cast<int64_t>(b);
}

float key_float(int64_t k) {
    const uint32_t b = k >= static_cast<int64_t>(0x80000000u)
                           ? static_cast<uint32_t>(k - static_cast<int64_t>(0x80000000u))
                           : 0x80000000u | static_cast<uint32_t>(static_cast<int64_t>(0x7fffffffu) - k);
    float x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

uint32_t bits_of(float x) {
    uint32_t b;
    std::memcpy(&b, &x, sizeof b);
    return b;
}

float float_of(uint32_t b) {
    float x;
    std::memcpy(&x, &b, sizeof x);
    return x;
}

// A box of a footprint level: element `index` of a pair-SoA table.
struct FBox {
    float lo[3], hi[3], K;
    int32_t index;
};

FBox fbox_of(const std::vector<float>& table, int32_t i) {
    const float* t = &table[static_cast<size_t>(i / 2) * 16];
    const int e = i % 2;
    return FBox{{t[0 + e], t[2 + e], t[4 + e]}, {t[6 + e], t[8 + e], t[10 + e]}, t[12 + e], i};
}

bool group_has_members(const CullTables& ct, int32_t gi) {
    bool members = false;
    for (int k = 0; k < 4; k++) members |= ct.index[(ct.nbig + gi) * 4 + k] >= 0;
    return members;
}

// The boxes of a level that have members (a padding box never gets a bit): the hierarchy groups
// (per = 1) or the nodes (per = kNodeGroups), exactly as uploaded.
std::vector<FBox> boxes_with_members(const CullTables& ct, int per) {
    std::vector<FBox> out;
    for (int32_t i = 0; i < ct.ngroups / per; i++) {
        bool members = false;
        for (int32_t gi = i * per; gi < (i + 1) * per; gi++) members |= group_has_members(ct, gi);
        if (members) out.push_back(fbox_of(per == 1 ? ct.bound : ct.node, i));
    }
    return out;
}

// One pair of footprint tables (axis a: A at tab, B at tab + n * words) by the rule of
// cluster.hpp: per cell i of n, with ue(i) the largest and le(i) the smallest float of the cell
// by the kernel's own cell function and g = 8u |e| + 2^-100,
//   A[i] = boxes with lo <= ue(i) + g,   B[i] = boxes with hi >= le(i) - g     (in double).
// Masks of `words` words (low first), bit = the box's index (none from 32 * words on).
void fill_masks(const std::vector<FBox>& boxes, int a, const float so[2], int n, int words,
                uint32_t* tab) {
    uint32_t* A = tab;
    uint32_t* B = tab + static_cast<size_t>(n) * words;
    const double inf = std::numeric_limits<double>::infinity();
    double prev_ue = -inf;  // the largest float of the cell before
    for (int i = 0; i < n; i++) {
        double ue = inf;
        if (i < n - 1) {  // the largest float whose cell is <= i: the cell never falls as x rises
            int64_t lo = float_key(-std::numeric_limits<float>::infinity());
            int64_t hi = float_key(std::numeric_limits<float>::infinity());
            while (hi - lo > 1) {  // cell(lo) <= i < cell(hi)
                const int64_t mid = lo + (hi - lo) / 2;
                (footprint_cell_n(key_float(mid), so, n) <= i ? lo : hi) = mid;
            }
            ue = key_float(lo);
        }
        // the smallest float of cell i is the one after prev_ue; comparing against prev_ue
        // itself only widens the mask
        const double le = prev_ue;
        const double up = ue + (8.0 * kU * std::fabs(ue) + 0x1p-100);
        const double dn = le - (8.0 * kU * std::fabs(le) + 0x1p-100);
        for (const FBox& b : boxes) {
            if (b.index >= 32 * words) continue;
            const uint32_t bit = 1u << (b.index & 31);
            if (static_cast<double>(b.lo[a]) <= up) A[words * i + (b.index >> 5)] |= bit;
            if (static_cast<double>(b.hi[a]) >= dn) B[words * i + (b.index >> 5)] |= bit;
        }
        prev_ue = ue;
    }
}

}  // namespace

int group_footprint_cells(int32_t ngroups) {
    if (ngroups <= 0) return 0;
    const int node_tables = 4 * kFootprintCells * (ngroups > 128 ? 4 : 2);
    return (ngroups / kNodeGroups * 336 + node_tables) / 64;
}

int footprint_cell_n(float x, const float so[2], int n) {
    const float f = std::fmaf(x, so[0], so[1]);
    const float c = std::fmin(std::fmax(f, 0.0f), static_cast<float>(n - 1));
    return static_cast<int>(c);  // truncation, as v_cvt_u32_f32
}

void summary_of_tables(const vcrt_sphere* s, int32_t count, const CullTables& ct,
                       SceneSummary& m) {
    m = SceneSummary{};
    for (int a = 0; a < 3; a++) {
        m.lo_min[a] = kKeyPosInf;
        m.hi_max[a] = kKeyNegInf;
    }
    m.ylo_max = kKeyNegInf;
    m.yhi_min = kKeyPosInf;
    m.bounded = m.radii_safe = 1u;
    for (int32_t i = 0; i < count; i++) {
        for (float v : {s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius})
            if (!(std::fabs(v) <= 0x1p30f)) m.bounded = 0u;  // also rejects NaN
        if (!(std::fabs(s[i].radius) >= 0x1p-40f && std::fabs(s[i].radius) <= 0x1p30f))
            m.radii_safe = 0u;
    }
    // the per-ray margin constants (tracer.hip, box_ray) over the hierarchy's spheres
    for (size_t e = static_cast<size_t>(ct.nbig) * 4; e < ct.index.size(); e++) {
        const int32_t j = ct.index[e];
        if (j < 0) continue;
        const double r = std::fabs(static_cast<double>(s[j].radius));
        m.rmax = std::max(m.rmax, r);
        double c2 = 0.0;
        for (int a = 0; a < 3; a++) {
            const double c = s[j].center[a];
            c2 += c * c;
            m.lam = std::max(m.lam, std::fabs(c) + r);
        }
        m.c2max = std::max(m.c2max, c2);
    }
    const bool masks = ct.ngroups <= kGroupFootprintMaxGroups;
    for (const FBox& b : boxes_with_members(ct, 1)) {
        m.boxes++;
        for (int a = 0; a < 3; a++) {
            m.lo_min[a] = std::min(m.lo_min[a], float_order_key(bits_of(b.lo[a])));
            m.hi_max[a] = std::max(m.hi_max[a], float_order_key(bits_of(b.hi[a])));
        }
        m.ylo_max = std::max(m.ylo_max, float_order_key(bits_of(b.lo[1])));
        m.yhi_min = std::min(m.yhi_min, float_order_key(bits_of(b.hi[1])));
        if (masks) m.group_real[b.index >> 5] |= 1u << (b.index & 31);
        if (std::isinf(b.K)) {
            if (masks) m.group_always[b.index >> 5] |= 1u << (b.index & 31);
        } else {
            m.group_kmax = std::max(m.group_kmax, bits_of(b.K));
        }
    }
    for (const FBox& b : boxes_with_members(ct, kNodeGroups)) {
        m.node_real |= b.index < 32 ? 1u << b.index : 0u;
        if (std::isinf(b.K))
            m.node_always |= b.index < 32 ? 1u << b.index : 0u;
        else
            m.node_kmax = std::max(m.node_kmax, bits_of(b.K));
    }
}

void scalars_of_summary(const SceneSummary& m, CullTables& out) {
    // sqrt rises with its argument, so the largest |c| is the root of the largest |c|^2
    out.margin[0] = round_up(std::sqrt(m.c2max) * (1.0 + 1e-6));
    out.margin[1] = round_up(m.rmax * m.rmax * (1.0 + 1e-6));
    out.margin[2] = round_up(m.lam * (1.0 + 1e-6));
    out.margin[3] = 0.0f;
    out.fp_always = 0xffffffffu;
    if (m.boxes == 0) return;
    double xlo[3], xhi[3];
    for (int a = 0; a < 3; a++) {
        xlo[a] = float_of(float_order_bits(m.lo_min[a]));
        xhi[a] = float_of(float_order_bits(m.hi_max[a]));
    }
    // The shared y slab: do all boxes with members have the same finite y extent, bit for bit?
    // (Padding boxes, the far point, are left out: their groups hold no member a ray can accept.)
    // A node's or chunk's y extent is the smallest lo and the largest hi of its groups', so the
    // group boxes decide for every level.
    const bool one_y = m.lo_min[1] == m.ylo_max && m.hi_max[1] == m.yhi_min &&
                       std::isfinite(xlo[1]) && std::isfinite(xhi[1]);
    // VCRT_SLAB=0 keeps the three-axis box tests (A/B and tests)
    const char* slab_env = std::getenv("VCRT_SLAB");
    if (one_y && !(slab_env && std::atoi(slab_env) == 0)) {
        out.slab = true;
        out.slab_lohi[0] = static_cast<float>(xlo[1]);
        out.slab_lohi[1] = static_cast<float>(xhi[1]);
    }
    const bool coords_ok = out.margin[2] >= 0x1p-20f;
    // scale and offset of n cells over [xlo, xhi] of axis a; false: the cells cannot describe it
    auto cells = [&](int a, int n, float so[2]) {
        const double w = xhi[a] - xlo[a];
        so[0] = static_cast<float>(n / w);
        so[1] = static_cast<float>(-xlo[a] * static_cast<double>(so[0]));
        return w > 0.0 && std::isnormal(so[0]) && std::isfinite(so[1]);
    };
    // The group-level tables (fact (5g)). A scene the cells cannot describe (a degenerate extent,
    // a coordinate bound below the 2^-20 of the proof) keeps every group with members for every
    // ray, as the node tables do.
    const int n = group_footprint_cells(out.ngroups);
    if (out.ngroups <= kGroupFootprintMaxGroups && n >= 2) {
        out.gf_cells = n;
        // one height: the same y extent in every group box with members, bit for bit (whatever
        // VCRT_SLAB says: that only chooses how box tests are evaluated)
        out.gf_one_height = one_y;
        const char* env = std::getenv("VCRT_GROUP_FOOT");
        out.gf_ok = one_y && !(env && std::atoi(env) == 0);
        out.gf_keep_all = !(coords_ok && cells(0, n, out.gf_x) && cells(2, n, out.gf_z));
        if (out.gf_keep_all) {
            std::memcpy(out.gf_always, m.group_real, sizeof(out.gf_always));
            out.gf_x[0] = out.gf_z[0] = 1.0f;
            out.gf_x[1] = out.gf_z[1] = 0.0f;
        } else {
            std::memcpy(out.gf_always, m.group_always, sizeof(out.gf_always));
            out.gf_k2 = round_up(2.0 * static_cast<double>(float_of(m.group_kmax)));
        }
    }
    // The node tables (cluster.hpp).
    out.fp_y[0] = static_cast<float>(xlo[1]);  // box coordinates: exact
    out.fp_y[1] = static_cast<float>(xhi[1]);
    out.fp_k2 = round_up(2.0 * static_cast<double>(float_of(m.node_kmax)));
    out.fp_ok = out.ngroups / kNodeGroups <= 32 && coords_ok && cells(0, kFootprintCells, out.fp_x) &&
                cells(2, kFootprintCells, out.fp_z);
    if (!out.fp_ok) {
        out.fp_x[0] = out.fp_z[0] = 1.0f;
        out.fp_x[1] = out.fp_z[1] = 0.0f;
        return;
    }
    out.fp_always = m.node_always;
}

void fill_footprints(CullTables& out) {
    if (out.gf_cells > 0) {
        const int n = out.gf_cells;
        out.gf_tab.assign(static_cast<size_t>(16) * n, 0u);
        if (out.gf_keep_all) {
            for (size_t i = 0; i < out.gf_tab.size(); i++) out.gf_tab[i] = out.gf_always[i & 3];
        } else {
            const std::vector<FBox> gb = boxes_with_members(out, 1);
            fill_masks(gb, 0, out.gf_x, n, 4, &out.gf_tab[0]);
            fill_masks(gb, 2, out.gf_z, n, 4, &out.gf_tab[static_cast<size_t>(2) * n * 4]);
        }
    }
    // The footprint tables (cluster.hpp): the node boxes exactly as uploaded, compared in double
    // with the exact edges of the kernel's own cell function.
    constexpr int N = kFootprintCells;
    out.fp_tab.assign(4 * N, 0xffffffffu);
    if (!out.fp_ok) return;
    out.fp_tab.assign(4 * N, 0u);
    const std::vector<FBox> nb = boxes_with_members(out, kNodeGroups);
    fill_masks(nb, 0, out.fp_x, N, 1, &out.fp_tab[0]);
    fill_masks(nb, 2, out.fp_z, N, 1, &out.fp_tab[2 * N]);
}

bool choose_grouping(const vcrt_sphere* s, int32_t count, CullTables& out) {
    out = CullTables{};
    if (count < 16) return false;
    for (int32_t i = 0; i < count; i++)
        for (float v : {s[i].center[0], s[i].center[1], s[i].center[2], s[i].radius})
            if (!(std::fabs(v) <= 0x1p30f)) return false;

    // Very large spheres (the ground) would inflate any group they join: a sphere is big when
    // its radius exceeds both 8x the median and 5% of the extent of all centres; at most the
    // 64 largest go to the big list (tested for every ray), the rest stay in the hierarchy.
    std::vector<float> radii(count);
    for (int32_t i = 0; i < count; i++) radii[i] = std::fabs(s[i].radius);
    std::vector<float> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + count / 2, sorted.end());
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        lo[a] = std::numeric_limits<double>::infinity();
        hi[a] = -lo[a];
    }
    for (int32_t i = 0; i < count; i++)
        for (int a = 0; a < 3; a++) {
            lo[a] = std::min(lo[a], static_cast<double>(s[i].center[a]));
            hi[a] = std::max(hi[a], static_cast<double>(s[i].center[a]));
        }
    const double extent = std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) +
                                    (hi[1] - lo[1]) * (hi[1] - lo[1]) +
                                    (hi[2] - lo[2]) * (hi[2] - lo[2]));
    const double huge = std::max(8.0 * sorted[count / 2], 0.05 * extent);
    std::vector<int32_t> normal, big;
    for (int32_t i = 0; i < count; i++) (radii[i] > huge ? big : normal).push_back(i);
    if (big.size() > 64) {  // keep the 64 largest (ties by index), return the rest
        std::stable_sort(big.begin(), big.end(),
                         [&](int32_t x, int32_t y) { return radii[x] > radii[y]; });
        normal.insert(normal.end(), big.begin() + 64, big.end());
        big.resize(64);
        std::sort(big.begin(), big.end());
    }
    // The big list's last group has free slots when the big spheres are not a multiple of four;
    // the largest of the rest fill them (ties by index). Every ray tests that group's members
    // anyway, while in the hierarchy a large sphere inflates the boxes of its group, node and
    // chunk for every ray that passes near it: the final scene's big three (radius 1, beside 480
    // of radius 0.2) join the ground, C4 +9% (same bits). It also keeps the stress scene's
    // hierarchy (4096 random spheres) within the flat scans' 1024 16-bit groups.
    // VCRT_BIG_FILL=0 disables it (A/B).
    const size_t free_slots = (4 - big.size() % 4) % 4;
    const char* fill_env = std::getenv("VCRT_BIG_FILL");
    const bool fill = !(fill_env && std::atoi(fill_env) == 0);
    if (fill && !big.empty() && free_slots > 0 && normal.size() > free_slots) {
        std::stable_sort(normal.begin(), normal.end(),
                         [&](int32_t x, int32_t y) { return radii[x] > radii[y]; });
        big.insert(big.end(), normal.begin(), normal.begin() + free_slots);
        normal.erase(normal.begin(), normal.begin() + free_slots);
        std::sort(big.begin(), big.end());
        std::sort(normal.begin(), normal.end());
    }
    // Big spheres go to a short list the kernels test for every ray (they are hit by most);
    // the rest form the hierarchy: groups of 4, nodes of 8 groups, chunks of 64 groups.
    std::vector<Group> bigg, groups;
    if (!big.empty()) split(big, 0, big.size(), s, bigg);
    if (!normal.empty()) split(normal, 0, normal.size(), s, groups);
    // pad the hierarchy to whole nodes and an even node count (pair layout)
    while (groups.size() % (2 * kNodeGroups)) groups.push_back(Group{-1, -1, -1, -1});

    const size_t nbig = bigg.size(), ng = groups.size(), nall = nbig + ng;
    out.nbig = static_cast<int32_t>(nbig);
    out.ngroups = static_cast<int32_t>(ng);
    out.index.assign(nall * 4, -1);
    for (size_t gi = 0; gi < nall; gi++) {
        const Group& g = gi < nbig ? bigg[gi] : groups[gi - nbig];
        for (int k = 0; k < 4; k++) out.index[gi * 4 + k] = g[k];
    }
    return true;
}

bool build_cull_tables(const vcrt_sphere* s, int32_t count, CullTables& out) {
    if (!choose_grouping(s, count, out)) return false;
    tables_of_grouping(s, count, out);
    return true;
}

void tables_of_grouping(const vcrt_sphere* s, int32_t count, CullTables& out) {
    {  // everything but the grouping starts from its default
        CullTables fresh;
        fresh.nbig = out.nbig;
        fresh.ngroups = out.ngroups;
        fresh.index = std::move(out.index);
        out = std::move(fresh);
    }
    const size_t nbig = out.nbig, ng = out.ngroups, nall = nbig + ng;
    out.geom.assign(nall * 16, 0.0f);
    out.bound.assign(ng / 2 * 16, 0.0f);
    out.node.assign(ng / kNodeGroups / 2 * 16, 0.0f);
    for (size_t gi = 0; gi < nall; gi++) {
        // members: pair-SoA exactly as the linear table (r^2 = radius * radius in fp32)
        for (int k = 0; k < 4; k++) {
            float* base = &out.geom[gi * 16 + 8 * (k / 2)];
            const int e = k % 2;
            const int32_t j = out.index[gi * 4 + k];
            float cx = 0.f, cy = 0.f, cz = 0.f, r2 = -3.0e38f;
            if (j >= 0) {
                const vcrt_sphere& sp = s[j];
                cx = sp.center[0];
                cy = sp.center[1];
                cz = sp.center[2];
                r2 = sp.radius * sp.radius;
            }
            base[0 + e] = cx;
            base[2 + e] = cy;
            base[4 + e] = cz;
            base[6 + e] = r2;
        }
    }
    auto box_at = [&](size_t g0, size_t g1) {
        std::vector<int32_t> m;
        for (size_t gi = g0; gi < std::min(g1, ng); gi++)
            for (int k = 0; k < 4; k++)
                if (out.index[(nbig + gi) * 4 + k] >= 0) m.push_back(out.index[(nbig + gi) * 4 + k]);
        return box_of(s, m);
    };
    for (size_t gi = 0; gi < ng; gi++) put_box(out.bound, gi, box_at(gi, gi + 1));
    for (size_t ni = 0; ni < ng / kNodeGroups; ni++)
        put_box(out.node, ni, box_at(ni * kNodeGroups, (ni + 1) * kNodeGroups));
    // top level: one box per chunk of 64 groups (the kernels' unit of work per pass)
    const size_t nt = (ng + 63) / 64, nt2 = nt + (nt & 1);
    out.top.assign(nt2 / 2 * 16, 0.0f);
    for (size_t ti = 0; ti < nt2; ti++) put_box(out.top, ti, box_at(ti * 64, ti * 64 + 64));

    SceneSummary m;
    summary_of_tables(s, count, out, m);
    scalars_of_summary(m, out);
    fill_footprints(out);
}

int footprint_cell(float x, const float so[2]) {
    const float f = std::fmaf(x, so[0], so[1]);
    const float c = std::fmin(std::fmax(f, 0.0f), static_cast<float>(kFootprintCells - 1));
    return static_cast<int>(c);  // truncation, as v_cvt_u32_f32
}

}  // namespace vcrt
