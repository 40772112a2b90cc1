// Host side shared by the four skinny weight-streaming kernel families (skinny.hip: fp32, skinny_bf16.hip: bf16 operands): one
// instantiation table per family, out of which both the launch and the dynamic-LDS attribute come, and the LDS size of a launch.
// (The kernels' slice staging and cross-wave reductions are alike too, but stay written out in each kernel: as shared device
// helpers they moved the register allocation of most instantiations, profiles/skinny_codegen_after.txt.)
#pragma once
#include "common.h"

namespace mstts {

// ---- host side of a launch
// One instantiation of a kernel family: its exact trip count (0 = the guarded form that takes any) and whether rows 16..31 of the
// block exist.  Each family names every instantiation ONCE, in a table; skinny_pick launches out of that table and skinny_lds_attr
// prepares exactly that table, so no instantiation can be launched without its LDS attribute.
template <typename Fn>
struct SkinnyInst {
    int nit;
    bool two;
    Fn kernel;
};
#define SKINNY_ROWS(KERNEL, n) {n, true, KERNEL(n, true)}, {n, false, KERNEL(n, false)}
// the guard-free instantiation when the trip count is one the model's shapes produce, else the guarded one
template <typename Fn, size_t N>
static inline Fn skinny_pick(const SkinnyInst<Fn> (&table)[N], int nit, bool two) {
    Fn any = nullptr;
    for (const SkinnyInst<Fn>& k : table) {
        if (k.two != two) continue;
        if (k.nit == nit) return k.kernel;
        if (k.nit == 0) any = k.kernel;
    }
    return any;
}
template <typename Fn, size_t N>
static inline void skinny_lds_attr(const SkinnyInst<Fn> (&table)[N]) {
    for (const SkinnyInst<Fn>& k : table) hipFuncSetAttribute((const void*)k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}
// dynamic LDS of a launch: the [32, width (+ pad)] slice of elem_bytes elements, reused as red[4 waves][32][red_ld] floats
static inline size_t skinny_lds_bytes(int width, int pad, size_t elem_bytes, int red_ld) {
    const size_t slice = (size_t)32 * (width + pad) * elem_bytes, red = sizeof(float) * 4 * 32 * red_ld;
    return slice > red ? slice : red;
}

}  // namespace mstts
