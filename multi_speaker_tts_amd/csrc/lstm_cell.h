// The zoneout-LSTM cell of one (row, unit), forward and backward: the ONE statement of ZoneoutLSTMCell.py:228-271 in the library.  Every
// kernel that updates a cell (the pointwise kernels of elementwise.hip, the fused cell of cell.hip, the persistent loops of persist*.hip)
// calls these two.  They take FINISHED gate pre-activations: the sum of slabs, input product and bias is the call site's, in the call
// site's order.  The length rule of dynamic_rnn (a dead row keeps its states, emits 0, saves zero activations and c_raw = c_prev) is the
// call site's as well: what is stored differs by kernel.
#pragma once
#include "common.h"

namespace mstts {

struct CellOut { float si, tj, sf, so, c, m; };      // sig i, tanh j, sig (f + 1), sig o; raw cell state; cell output
// gates i, j, f, o (forget bias 1.0 added here); zoneout as state' = k (new - old) + old with k = (1 - z) * keep-mask in training
// (:266-271) and k = 1 - z at inference (:259-264).  Updates the carried states cs / hs.
__device__ __forceinline__ CellOut lstm_cell_fwd(float gi, float gj, float gf, float go, float& cs, float& hs, float kc, float kh) {
    CellOut o;
    o.si = sigmoidf_(gi); o.tj = tanhf_(gj); o.sf = sigmoidf_(gf + 1.0f); o.so = sigmoidf_(go);
    o.c = o.sf * cs + o.si * o.tj;
    o.m = o.so * tanhf_(o.c);
    hs = kh * (o.m - hs) + hs;
    cs = kc * (o.c - cs) + cs;
    return o;
}

struct CellGrad { float i, j, f, o; };               // gradients of the four gate pre-activations
// dm = gradient of the cell output m (without the zoned-state path), dhs / dcs = gradients of the zoned states h' / c', mh / mc = d h'/d m
// and d c'/d c (the forward's kh / kc).  Returns the gate gradients, updates the carried state gradients to those of the PREVIOUS step's
// states (direct zoneout paths only; the recurrent product's part is added by the caller).
__device__ __forceinline__ CellGrad lstm_cell_bwd(float dm, float& dhs, float& dcs, float si, float tj, float sf, float so, float c, float cp,
                                                  float mh, float mc) {
    dm += mh * dhs;
    const float tc = tanhf_(c);
    const float dc = dm * so * (1.f - tc * tc) + mc * dcs;
    CellGrad g;
    g.i = dc * tj * si * (1.f - si);
    g.j = dc * si * (1.f - tj * tj);
    g.f = dc * cp * sf * (1.f - sf);
    g.o = dm * tc * so * (1.f - so);
    dcs = dcs * (1.f - mc) + dc * sf;
    dhs = dhs * (1.f - mh);
    return g;
}

}  // namespace mstts
