// espcn_f16_d2s_store.h -- the store side of the fp16 depth-to-space tails, #included by espcn_f16_b_body.h (kernel B16<R>) and espcn_f16_wide_b_body.h
// (kernel B16 wide<R>): bias / BN / act -> half, tanh -> half, then the half, 8-bit or 16-bit frame store of the R consecutive output pixels a lane
// owns (the R = 3 byte packing, the 6-byte 16-bit stores, quantize_u8 / quantize_u16).  One text, so the two kernels cannot drift apart.
// In scope: R, SIMPLE, the type TOut, G, the kernel arguments p, qout16, y, and n, x0, y0, wv, px, g, acc[G] (row 4*dy + dx = channel R*dy + dx:
// group gi = row 2*wv + (gi >> 1), columns 16*(gi & 1) .. + 15 of the tile), sc[4], sh[4].
    // ---- epilogue: bias/BN/act -> half, tanh -> half; lane (px, g < R) holds output row R*gy + g, columns R*gx .. R*gx + R-1
    TOut* yn = y + static_cast<size_t>(n) * (R * p.H) * (R * p.W);
    [[maybe_unused]] const bool dwordRows = (p.W & 3) == 0; // R = 3, bytes: every pixel quad starts on a 4-byte boundary
#pragma unroll
    for (int gi = 0; gi < G; ++gi) {
        const int gy = y0 + wv * 2 + (gi >> 1), gx = x0 + (gi & 1) * 16 + px;
        const bool ok = g < R && gy < p.H && gx < p.W;
        _Float16 o[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const _Float16 c3 = static_cast<_Float16>(apply_act<SIMPLE>(p.act, fmaf(acc[gi][r], sc[r], sh[r]), 0.0f)); // what the Subpixel plan would read
            o[r] = static_cast<_Float16>(fast_tanh(static_cast<float>(c3)));
        }
        TOut* dst = yn + static_cast<size_t>(R * gy + g) * (R * p.W) + R * gx;
        if constexpr (FrameBits<TOut>::value == 16) { // the half output's store layout, 2-byte elements
            unsigned q[R];
#pragma unroll
            for (int r = 0; r < R; ++r) q[r] = quantize_u16(static_cast<float>(o[r]), qout16.scale, qout16.offset, qout16.maxval) << qout16.shift;
            if constexpr (R == 4) {
                if (ok) *reinterpret_cast<uint2*>(dst) = make_uint2(q[0] | (q[1] << 16), q[2] | (q[3] << 16));
            } else if constexpr (R == 2) {
                if (ok) *reinterpret_cast<unsigned*>(dst) = q[0] | (q[1] << 16);
            } else if (ok) { // 6 bytes at a 2-byte aligned address: 4 + 2 or 2 + 4
                if ((reinterpret_cast<uintptr_t>(dst) & 2) == 0) {
                    *reinterpret_cast<unsigned*>(dst) = q[0] | (q[1] << 16);
                    dst[2] = static_cast<TOut>(q[2]);
                } else {
                    dst[0] = static_cast<TOut>(q[0]);
                    *reinterpret_cast<unsigned*>(dst + 1) = q[1] | (q[2] << 16);
                }
            }
        } else if constexpr (FrameBits<TOut>::value == 8) {
            unsigned v = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) v |= quantize_u8(static_cast<float>(o[r]), p.qscale, p.qoffset) << (8 * r);
            if constexpr (R == 4) {
                if (ok) *reinterpret_cast<unsigned*>(dst) = v;
            } else if constexpr (R == 2) {
                if (ok) *reinterpret_cast<unsigned short*>(dst) = static_cast<unsigned short>(v);
            } else {
                const unsigned nb = __shfl_down(v, 1); // the right neighbour's three bytes (every lane takes part)
                const int j = px & 3;
                if (dwordRows) { // W % 4 == 0: a quad is inside the image or outside it as a whole, and starts on a 4-byte boundary
                    if (ok && j < 3) *reinterpret_cast<unsigned*>(dst + j) = (v >> (8 * j)) | (nb << (24 - 8 * j));
                } else if (ok) {
                    dst[0] = static_cast<unsigned char>(v);
                    dst[1] = static_cast<unsigned char>(v >> 8);
                    dst[2] = static_cast<unsigned char>(v >> 16);
                }
            }
        } else {
            if constexpr (R == 4) {
                if (ok) *reinterpret_cast<f16x4*>(dst) = f16x4{o[0], o[1], o[2], o[3]};
            } else if constexpr (R == 2) {
                if (ok) *reinterpret_cast<f16x2*>(dst) = f16x2{o[0], o[1]};
            } else if (ok) { // 6 bytes at a 2-byte aligned address: 4 + 2 or 2 + 4
                if ((reinterpret_cast<uintptr_t>(dst) & 2) == 0) {
                    *reinterpret_cast<f16x2*>(dst) = f16x2{o[0], o[1]};
                    dst[2] = static_cast<TOut>(o[2]);
                } else {
                    dst[0] = static_cast<TOut>(o[0]);
                    *reinterpret_cast<f16x2*>(dst + 1) = f16x2{o[1], o[2]};
                }
            }
        }
    }
