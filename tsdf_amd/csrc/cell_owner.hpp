// Which dual cell OWNS a sample: the cell whose 8 voxels the reference's trilinearly_interpolate reads for it, decided exactly, in
// registers, from products the reference itself forms.  Plain C++ for both sides, like cell_boxes.hpp: cast_cells_kernel runs cell_owns
// on the GPU, tsdf_selftest_cell_owner runs it on the host beside a restatement of the reference's own choice (reference_lower below:
// voxel_for_point + centre_of_voxel_at as trilinear() in raycast_sample.hpp inlines them) and tests/test_cell_owner_host.py compares
// the two on every face of every cell, a few ulps either side, with no GPU.
//
// The reference, per axis (raycast_sample.hpp:85-113; p the sample's coordinate, vs the voxel edge, both fp32, every operation rounded
// on its own -- the translation units are compiled with -ffp-contract=off):
//     a = p, but clamp if p >= max, 0 if p < 0;   v = floor(a / vs);   c = (v + 0.5f) * vs;   lower = max(p < c ? v - 1 : v, 0)
// The cells' kernel offers cell l (integer 0 <= l, l + 1 < size: `valid`) only samples that pass its coarse test, |p / vs - (l + 1)| <=
// 0.5 + eps + a few 1e-5 of arithmetic (eps <= 2e-3 for the largest grid there is, 65 535 voxels: cell_guard_eps): call the band B.
//
// 1. v is l or l + 1 for every p in B.  The exact quotient p / vs lies in [l + 0.497, l + 1.503].  The IEEE division rounds it to the
//    nearest float, which is monotone and leaves the integers l, l + 1, l + 2 (floats themselves) where they are: the rounded quotient
//    lies in [l + 0.49, l + 1.51] and its floor is l or l + 1.  The fast division (div_by<FASTDIV>: q0 = p y, q = fma(fma(-vs, q0, p),
//    y, q0), y = RN(1 / vs)) is used only for a vs for which the volume has checked it against the IEEE quotient on every numerator of
//    its domain, and takes the IEEE division outside that domain: it IS the IEEE quotient.  (Unverified it would do as well: it is good
//    to 2 ulps of a quotient below 2^16, under 1e-2 of a voxel against a margin of 0.49; the test runs that form too.)
//    With v = l:      lower = l  iff  !(p < (l + 0.5f) * vs); and p < (l + 1.5f) * vs holds anyway (p / vs < l + 1.01).
//    With v = l + 1:  lower = l  iff    p < (l + 1.5f) * vs;  and p >= (l + 0.5f) * vs holds anyway (p / vs > l + 0.99).
//    Either way  lower == l  <=>  (l + 0.5f) * vs <= p < (l + 1.5f) * vs: cell_owns.  Its two products are the reference's c for v = l
//    and for v = l + 1, rounded as the reference rounds them; the comparisons are exact.  Consecutive cells share a product, so every
//    p is owned by exactly one cell of an axis.
// 2. The clamps cannot fire for a valid cell's owned sample.  p >= (l + 0.5f) * vs > 0: not `p < 0`, and lower >= 0 without the max.
//    p < (l + 1.5f) * vs <= (size - 0.5) * vs (1 + 2^-23), half a voxel under max = RN(size * vs): not `p >= max`; and v <= l + 1 <
//    size, so the reference does not leave through its off-grid return.  l + 1 < size also means none of the 8 taps is clamped
//    (tsdf_value_at): the taps are the cell's own 8 voxels, the ones the brick's turn holds.
// 3. l + 0.5f and l + 1.5f are exact: l is an integer below 2^16 (the volume refuses a larger axis), so l + 1.5 has at most 16 bits in
//    front of the point and one behind it, and the int -> float conversion of v in the reference's (v + 0.5f) is exact as well.
//
// So an owned sample takes the interior expression -- the reference's u = (p - (l + 0.5f) * vs) / vs on the reference's taps -- and a
// sample that is not owned is the owning cell's: that cell's task offers it too (its own band holds the sample) and evaluates it if the
// cell is mixed.  What this does not change: a cell none of whose voxels is <= kCellPositive has no task, and its samples are taken to
// be positive.  For a sample within rounding of a face, u can leave [0, 1] by l 2^-23 (the two products are each rounded), so that
// claim leans on the cell's voxels not differing by a factor of 1 / that; before, a mixed neighbour's task would still have evaluated
// such a sample, now only the owner does.
#pragma once
#include <cmath>
#include <cstdint>

#include "cell_boxes.hpp"   // TSDF_BOX_HD

namespace tsdf {

// p is owned, along one axis, by the cell whose lower voxel is l (lf = (float)l): see above.  Two products, two compares, no load.
TSDF_BOX_HD inline bool cell_owns(float p, float lf, float vs) {
    return p >= (lf + 0.5f) * vs && p < (lf + 1.5f) * vs;
}
TSDF_BOX_HD inline bool cell_owns(float px, float py, float pz, float lfx, float lfy, float lfz, float vsx, float vsy, float vsz) {
    return cell_owns(px, lfx, vsx) && cell_owns(py, lfy, vsy) && cell_owns(pz, lfz, vsz);
}

// The reference's choice of the lower tap along one axis, restated (trilinear(), raycast_sample.hpp:85-113): size voxels of edge vs.
// fast: the quotient as div_by<true> forms it inside its domain (|a| >= fast_min, finite), the IEEE quotient outside.  Returns -1
// where the reference leaves through its off-grid return.
TSDF_BOX_HD inline int reference_lower(float p, float vs, uint32_t size, bool fast, float fast_min) {
    const float max_ = (float)size * vs, clamp_ = max_ - (vs / 10.0f);
    float a = p;
    if (p >= max_) a = clamp_;
    if (p < 0.0f) a = 0.0f;
    float q = a / vs;
    if (fast && fabsf(a) >= fast_min && fabsf(a) < INFINITY) {
        const float y = 1.0f / vs, q0 = a * y;
        q = fmaf(fmaf(-vs, q0, a), y, q0);
    }
    const float fl = floorf(q);
    if (!(fl >= 0.0f && fl < (float)size)) return -1;
    const int v = (int)fl;
    const float c = (v + 0.5f) * vs + 0.0f;
    const int lower = (p < c) ? v - 1 : v;
    return lower > 0 ? lower : 0;
}

}  // namespace tsdf
