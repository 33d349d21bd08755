// conv3p_abi_blocks.hpp -- layers served in channel blocks: fp32 layers of more than 256 channels on the matrix-core
// kernels, fp64 layers outside the register shapes on the register kernels, and the fp64 36 -> 13 column split.
// Included by conv3p_abi.hip.
namespace {

// ----------------------------------------------------------------------------- what the blocked drivers share
// The op is linear in the input-channel blocks and independent over the output-channel blocks: a driver packs a block's
// rows and its filter block into scratch (zero-filled to the block kernel's shape), runs the block kernel on a copy of
// the Call with the block's shape, and adds the blocks' results in ascending order -- deterministic.
inline unsigned grid_1d(size_t n) { return capped_grid((n + 255) / 256, 4096); }
// dst [rows][ldp] = src[:, 0 .. cols) zero-filled to ldp columns
template <typename T> int pack_rows(const Call<T> &c, const T *src, int ld_s, T *dst, size_t rows, int cols, int ldp)
{
    if (cols < ldp) TRY(zero_async(dst, rows * (size_t)ldp * sizeof(T), c.s));
    hipLaunchKernelGGL(copy_cols_kernel<T>, dim3(grid_1d(rows * cols)), dim3(256), 0, c.s, src, dst, rows, cols, ld_s, ldp);
    return CONV3P_OK;
}
// wp [ntap][kwp][cwp] = filter[:, k0 .. k0 + kw, c0 .. c0 + cw) zero-filled.  kind: the profile kind the copy counts under
// (kNoKind: none -- the fp64 blocks' copies run under K_TRANSPOSE, by which the profile tells them from the register path)
template <typename T>
int pack_filter_block(const Call<T> &c, int kind, const T *filter, int k0, int kw, int c0, int cw, int kwp, int cwp, T *wp)
{
    const Dims &d = c.d;
    if (kw < kwp || cw < cwp) TRY(zero_async(wp, (size_t)d.ntap * kwp * cwp * sizeof(T), c.s));
    Scope sc(kind, c.s);
    hipLaunchKernelGGL(copy_block_kernel<T>, dim3(grid_1d((size_t)d.ntap * kw * cw)), dim3(256), 0, c.s,
                       filter + (size_t)k0 * d.Cout + c0, wp, d.ntap, kw, cw, (size_t)d.Cin * d.Cout, d.Cout, (size_t)kwp * cwp, cwp);
    return CONV3P_OK;
}
// ... and back: grad_filter[:, k0 .. k0 + kw, c0 .. c0 + cw) = dwp [ntap][kwp][cwp]
template <typename T>
void scatter_filter_block(const Call<T> &c, const T *dwp, int k0, int kw, int c0, int cw, int kwp, int cwp, T *grad_filter)
{
    const Dims &d = c.d;
    hipLaunchKernelGGL(copy_block_kernel<T>, dim3(grid_1d((size_t)d.ntap * kw * cw)), dim3(256), 0, c.s, dwp,
                       grad_filter + (size_t)k0 * d.Cout + c0, d.ntap, kw, cw, (size_t)kwp * cwp, cwp, (size_t)d.Cin * d.Cout, d.Cout);
}
// dst[:, 0 .. cols) = src[:, 0 .. cols) for the first block of a sum, += for the later ones
template <typename T> void sum_cols(const Call<T> &c, bool first, const T *src, int ld_s, T *dst, int ld_d, size_t rows, int cols)
{
    if (first) hipLaunchKernelGGL(copy_cols_kernel<T>, dim3(grid_1d(rows * cols)), dim3(256), 0, c.s, src, dst, rows, cols, ld_s, ld_d);
    else hipLaunchKernelGGL(add_cols_kernel<T>, dim3(grid_1d(rows * cols)), dim3(256), 0, c.s, src, dst, rows, cols, ld_s, ld_d);
}
// the Call of a (ci x co) block kernel over packed rows: no epilogue, nothing to add to
template <typename T> Call<T> block_call(const Call<T> &c, int ci, int co)
{
    Call<T> cp = c;
    cp.d.Cin = ci;
    cp.d.Cout = co;
    cp.act = false;
    cp.accum = false;
    cp.addend = nullptr;
    set_ld(cp, nullptr, ci, co);
    return cp;
}

// ----------------------------------------------------------------------------- layers of more than 256 channels
// A block of kw <= 256 channels is packed into rows of 128 or 256 floats, zero-filled past kw: every block then IS one of
// the instantiated shapes {128, 256}^2 with full rows (the kernels' fast path), whatever the layer's channel counts.
inline WideScratch carve_wide(const Call<float> &c, bool forward_only = false)
{
    const Dims &d = c.d;
    // (a forward-only workspace ends after the forward's part of the block scratch: the packs follow that; a cache sized
    // for the backward keeps ONE placement for both passes)
    const size_t slots = (size_t)d.B * c.L.pairs_per_cloud;
    const bool forward_part = forward_only && c.scratch < wide_scratch_bytes(d, slots);
    WideScratch w{};
    (void)carve_wide_scratch(d, slots, forward_part, c.L.partials, w);
    return w;
}

// out[:, c0 .. c0 + cw) = sum over the input-channel blocks of conv(input[:, k0 .. k0 + kw), filter[:, k-block, c-block]):
// every block runs on the matrix-core kernels from packed copies (the same geometry and record order for all of them),
// the blocks' results are added in ascending k0.
int wide_forward(const Call<float> &c, const Route &r, const float *input, const float *filter, float *output)
{
    const Dims &d = c.d;
    const size_t rows = (size_t)d.B * d.N;
    const WideScratch w = carve_wide(c, /*forward_only=*/true);
    bool have_order = c.order_ok[0];
    for (int c0 = 0; c0 < d.Cout; c0 += kWideBlk) {
        const int cw = d.Cout - c0 < kWideBlk ? d.Cout - c0 : kWideBlk, cwp = wide_pad(cw);
        for (int k0 = 0; k0 < d.Cin; k0 += kWideBlk) {
            const int kw = d.Cin - k0 < kWideBlk ? d.Cin - k0 : kWideBlk, kwp = wide_pad(kw);
            TRY(pack_rows(c, input + k0, d.Cin, w.xp, rows, kw, kwp));
            TRY(pack_filter_block(c, kNoKind, filter, k0, kw, c0, cw, kwp, cwp, w.wp));
            Call<float> cp = block_call(c, kwp, cwp);
            cp.order_ok[0] = have_order;
            TRY(deep_shape(kwp, cwp)->forward(cp, r, w.xp, w.wp, w.zp));
            have_order = true;
            sum_cols(c, k0 == 0, w.zp, cwp, output + c0, d.Cout, rows, cw);
        }
    }
    return hip_ok();
}

// grad_input[:, k-block] = sum over the output-channel blocks (ascending c0) of the block's grad_input; every
// (k-block, c-block) pair gives its own block of grad_filter.
int wide_backward(const Call<float> &c, const Route &r, const float *grad_out, const float *input, const float *filter,
                  float *grad_input, float *grad_filter)
{
    const Dims &d = c.d;
    const size_t rows = (size_t)d.B * d.N;
    const WideScratch w = carve_wide(c);
    bool have_order = c.order_ok[1];
    for (int k0 = 0; k0 < d.Cin; k0 += kWideBlk) {
        const int kw = d.Cin - k0 < kWideBlk ? d.Cin - k0 : kWideBlk, kwp = wide_pad(kw);
        TRY(pack_rows(c, input + k0, d.Cin, w.xp, rows, kw, kwp));
        for (int c0 = 0; c0 < d.Cout; c0 += kWideBlk) {
            const int cw = d.Cout - c0 < kWideBlk ? d.Cout - c0 : kWideBlk, cwp = wide_pad(cw);
            TRY(pack_rows(c, grad_out + c0, d.Cout, w.yp, rows, cw, cwp));
            TRY(pack_filter_block(c, kNoKind, filter, k0, kw, c0, cw, kwp, cwp, w.wp));
            Call<float> cp = block_call(c, kwp, cwp);
            cp.order_ok[1] = have_order;
            TRY(deep_shape(kwp, cwp)->backward(cp, r, w.yp, w.xp, w.wp, w.zp, w.dwp));
            have_order = true;
            sum_cols(c, c0 == 0, w.zp, kwp, grad_input + k0, d.Cin, rows, kw);
            scatter_filter_block(c, w.dwp, k0, kw, c0, cw, kwp, cwp, grad_filter);
        }
    }
    return hip_ok();
}

// ----------------------------------------------------------------------------- fp64 layers outside the register-path shapes
inline F64Scratch carve_f64(const Call<double> &c)
{
    F64Scratch w{};
    (void)carve_f64_scratch(c.d, c.L.partials, w);
    return w;
}

// out[:, c-block] = sum over the input-channel blocks (ascending) of the block kernel's result
int f64_blocked_forward(const Call<double> &c, const Route &r, const double *input, const double *filter, double *output)
{
    const Dims &d = c.d;
    const size_t rows = (size_t)d.B * d.N;
    const F64Scratch w = carve_f64(c);
    const Call<double> cp = block_call(c, kF64FwdKi, kF64FwdCo);
    for (int k0 = 0; k0 < d.Cin; k0 += kF64FwdKi) {
        const int kw = d.Cin - k0 < kF64FwdKi ? d.Cin - k0 : kF64FwdKi;
        TRY(pack_rows(c, input + k0, d.Cin, w.xp, rows, kw, kF64FwdKi));
        for (int c0 = 0; c0 < d.Cout; c0 += kF64FwdCo) {
            const int cw = d.Cout - c0 < kF64FwdCo ? d.Cout - c0 : kF64FwdCo;
            TRY(pack_filter_block(c, K_TRANSPOSE, filter, k0, kw, c0, cw, kF64FwdKi, kF64FwdCo, w.wp));
            TRY((launch_forward<double, kF64FwdKi, kF64FwdCo>(cp, r.lds, false, w.xp, w.wp, w.yp)));
            sum_cols(c, k0 == 0, w.yp, kF64FwdCo, output + c0, d.Cout, rows, cw);
        }
    }
    return hip_ok();
}

// grad_input[:, k-block] = sum over the output-channel blocks (ascending) of the block's grad_input; every block pair
// gives its own block of grad_filter (per-workgroup partials, reduced in fixed order).  BCO: output channels per block.
template <int BCO>
int f64_blocked_backward_co(const Call<double> &c, const Route &r, const double *grad_out, const double *input,
                            const double *filter, double *grad_input, double *grad_filter)
{
    const Dims &d = c.d;
    const size_t rows = (size_t)d.B * d.N, nwb = (size_t)d.ntap * kF64BwdKi * BCO;
    const int nslots = (int)grid_of(make_blockmap(d));
    const F64Scratch w = carve_f64(c);
    const Call<double> cp = block_call(c, kF64BwdKi, BCO);
    for (int k0 = 0; k0 < d.Cin; k0 += kF64BwdKi) {
        const int kw = d.Cin - k0 < kF64BwdKi ? d.Cin - k0 : kF64BwdKi;
        TRY(pack_rows(c, input + k0, d.Cin, w.xp, rows, kw, kF64BwdKi));
        for (int c0 = 0; c0 < d.Cout; c0 += BCO) {
            const int cw = d.Cout - c0 < BCO ? d.Cout - c0 : BCO;
            TRY(pack_rows(c, grad_out + c0, d.Cout, w.yp, rows, cw, BCO));
            TRY(pack_filter_block(c, K_TRANSPOSE, filter, k0, kw, c0, cw, kF64BwdKi, BCO, w.wp));
            TRY((launch_backward<double, kF64BwdKi, BCO>(cp, r.lds, w.yp, w.xp, w.wp, w.zp, w.parts)));
            {
                Scope sc(K_REDUCE, c.s);
                hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)((nwb + kReduceW - 1) / kReduceW)), dim3(1024), 0, c.s, w.parts,
                                   nslots, nwb, w.dwp);
            }
            sum_cols(c, c0 == 0, w.zp, kF64BwdKi, grad_input + k0, d.Cin, rows, kw);
            scatter_filter_block(c, w.dwp, k0, kw, c0, cw, kF64BwdKi, BCO, grad_filter);
        }
    }
    return hip_ok();
}
// r.co: output channels per block, the widest whose dense G fits LDS (plan_backward)
int f64_blocked_backward(const Call<double> &c, const Route &r, const double *grad_out, const double *input,
                         const double *filter, double *grad_input, double *grad_filter)
{
    if (r.co == kF64BwdCo) return f64_blocked_backward_co<kF64BwdCo>(c, r, grad_out, input, filter, grad_input, grad_filter);
    if (r.co == 4) return f64_blocked_backward_co<4>(c, r, grad_out, input, filter, grad_input, grad_filter);
    return f64_blocked_backward_co<2>(c, r, grad_out, input, filter, grad_input, grad_filter);
}

// ----------------------------------------------------------------------------- the fp64 36 -> 13 column split
// fp64 36 -> 13 (the scene_seg head in double precision): the backward kernel's G matrix (27 x 13 rows of 64 doubles)
// plus the transposed filter do not fit LDS, and the generic kernels take 37 ms for it.  The op is linear in the
// output channels, so it runs as three passes of the SAME register-path kernel over column blocks of 5 + 4 + 4
// output channels: grad_out is read through its row stride from a column offset, the filter block is packed into
// scratch, every pass adds its grad_input contribution to the previous ones (the SELU epilogue, if any, in the last
// pass), and the grad_filter blocks are reduced and scattered back.  Deterministic like the single-pass kernel.
// r.lds, r.lds4: the kernel's LDS for the 5- and 4-column passes.
template <typename T>
int backward_split_36_13(const Call<T> &c, const Route &r, const T *grad_out, const T *input, const T *filter,
                         T *grad_input, T *grad_filter)
{
    if constexpr (sizeof(T) != 8) {
        return CONV3P_ERR_UNSUPPORTED;   // (never planned)
    } else {
        const Dims &d = c.d;
        const int widths[3] = {5, 4, 4};
        const int nslots = (int)grid_of(make_blockmap(d));
        const size_t rows = (size_t)d.ntap * d.Cin;       // the filter as a matrix [ntap * Cin][Cout]: a column block is full rows
        const size_t nwp_max = rows * 5;
        T *region = c.L.partials;                         // [nslots][rows * width] per pass (sized for 13 columns)
        T *Wp = region + (size_t)nslots * nwp_max;        // packed filter block
        T *Wd = Wp + nwp_max;                             // its grad_filter block
        int c0 = 0;
        for (int p = 0; p < 3; ++p) {
            const int cw = widths[p];
            const size_t nwp = rows * cw;
            TRY(pack_rows(c, filter + c0, d.Cout, Wp, rows, cw, cw));
            Call<T> cp = c;   // (the feature tensors keep their row strides: only the filter is packed)
            cp.d.Cout = cw;
            cp.accum = p > 0;
            cp.act = c.act && p == 2;
            cp.addend = p == 2 ? c.addend : nullptr;
            TRY((cw == 5 ? launch_backward<T, 36, 5>(cp, r.lds, grad_out + c0, input, Wp, grad_input, region)
                         : launch_backward<T, 36, 4>(cp, r.lds4, grad_out + c0, input, Wp, grad_input, region)));
            {
                Scope sc(K_REDUCE, c.s);
                hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((unsigned)((nwp + kReduceW - 1) / kReduceW)), dim3(1024), 0, c.s, region,
                                   nslots, nwp, Wd);
            }
            sum_cols(c, true, Wd, cw, grad_filter + c0, d.Cout, rows, cw);
            c0 += cw;
        }
        return hip_ok();
    }
}

}  // namespace
