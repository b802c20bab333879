// Descriptor matching: for every image pair the nearest and second nearest
// descriptor of each keypoint, the ratio / distance / cross-check tests and the
// compacted matches, on the device.  The reference ships matching files and
// nothing that produces them; this is the stage in front of sfm_merge_tracks.
//
// Distances are exact integers (include/sfmcore.h).  The bytes are biased by
// -128 into signed i8 (one XOR with 0x80; a common shift leaves ||a - b||^2
// unchanged) and dsq = ||a'||^2 + ||b'||^2 - 2 a'.b' with the products a'.b' on
// the i8 MFMA (v_mfma_i32_16x16x64_i8) and the norms computed once per call.
// Every term is below 2^22 in magnitude, so the int32 accumulation is exact.
//
//   k_md_norms   ||a'||^2 of every keypoint, 16 bytes per thread.
//   k_md_nn      (in match_common.hpp: retrieval.hip instantiates it too)
//                a workgroup of 4 waves owns MD_BM = 128 rows of the pair's
//                first image: each wave keeps the A fragments of its 32 rows in
//                registers for the whole kernel (lane l: row l & 15, bytes
//                16 (l >> 4) .. + 15 of each 64-byte k step).  The second
//                image's descriptors stream through LDS in tiles of MD_TN = 64
//                columns, double buffered (global -> registers before the
//                tile's products, registers -> the other buffer after them, one
//                barrier per tile), rows padded by 16 bytes so that the 16
//                rows one ds_read_b128 phase touches fall into distinct banks.
//                A and B use the same (lane, byte) -> k map, so the k order
//                inside a step cannot matter to the sum.  Of the 16 x 16 result
//                a lane holds column l & 15 and rows 4 (l >> 4) + 0..3: per
//                row it keeps the running minimum of w = ||b'||^2 - 2 a'.b'
//                (||a'||^2 is added at the end), the column of the minimum
//                and the second smallest w.  Columns arrive ascending, so a
//                strict < keeps the smaller index on a tie, and the second of
//                the (dsq, index) order is just the second smallest value:
//                m2 = med3(m1, m2, w).  The 16 lanes of a row are merged by
//                the same order at the end.  Columns past the image's end
//                carry a norm that no real w reaches.
//                The reverse nearest neighbours (nn_rev) are a second launch
//                with the pair's images swapped (see DESIGN.md for the
//                alternative measured).
//   k_md_accept  the tests of a keypoint; one fp64 product.
//   rocPRIM      an exclusive scan of the accept flags: each match's place.
//   k_md_write   match_start and the compacted matches.
//
// Integer minima and a scan: every output is the same from run to run.
#include "match_common.hpp"

using namespace sfm;

extern "C" int sfm_match_descriptors(const uint8_t *desc, int64_t n_kp, const int64_t *img_start, int32_t n_images,
                                     int32_t dim, const int32_t *pairs, int64_t P, double ratio, int32_t max_dsq,
                                     int32_t cross_check, int64_t capacity, int64_t *match_start, int32_t *match_a,
                                     int32_t *match_b, int32_t *match_dsq, int32_t *nn, int32_t *d1, int32_t *d2,
                                     int32_t *nn_rev, int device) {
    MdPlan plan;
    SFM_TRY(md_plan(desc, n_kp, img_start, n_images, dim, pairs, P, ratio, max_dsq, cross_check, capacity, match_start,
                    match_a, match_b, match_dsq, plan));
    const int64_t *row_off = plan.row_off(), *col_off = plan.col_off();
    const int64_t max_i = plan.max_i, max_j = plan.max_j;
    const double ratio_sq = ratio * ratio;

    match_start[0] = 0;
    if (P == 0) return 0;
    const int64_t n_rows = row_off[P], n_cols = col_off[P];
    const bool reverse = cross_check || nn_rev;

    ThreadCtx *c = thread_ctx(device);
    if (!c) return SFM_ERR_HIP;
    hipStream_t s = c->stream;
    size_t tmp_bytes = 0;
    SFM_TRY(md_scan_bytes(n_rows, s, tmp_bytes));

    Pack in(c->buf[0]), out(c->buf[1]), work(c->buf[2]);
    const auto i_desc = in.add<uint8_t>(n_kp * dim);
    const auto i_is = in.add<int64_t>(n_images + 1);
    const auto i_pairs = in.add<int32_t>(2 * P);
    const auto i_ro = in.add<int64_t>(P + 1), i_co = in.add<int64_t>(P + 1);
    const auto o_ms = out.add<int64_t>(P + 1);
    const auto o_a = out.add<int32_t>(n_rows), o_b = out.add<int32_t>(n_rows), o_dsq = out.add<int32_t>(n_rows);
    const auto o_nn = out.add<int32_t>(n_rows), o_d1 = out.add<int32_t>(n_rows), o_d2 = out.add<int32_t>(n_rows);
    const auto o_rev = out.add<int32_t>(reverse ? n_cols : 0);
    const auto w_norm = work.add<int32_t>(n_kp);
    const auto w_flag = work.add<int32_t>(n_rows + 1);  // a last 0, so that the scan's last entry is the total
    const auto w_place = work.add<int64_t>(n_rows + 1);
    const auto w_tmp = work.add<char>(tmp_bytes);
    SFM_TRY(in.reserve());
    SFM_TRY(out.reserve());
    SFM_TRY(work.reserve());

    CallTimer tm(c);
    SFM_TRY(tm.mark(s));
    SFM_TRY(in.upload(i_desc, desc, s));
    SFM_TRY(in.upload(i_is, img_start, s));
    SFM_TRY(in.upload(i_pairs, pairs, s));
    SFM_TRY(in.upload(i_ro, row_off, s));
    SFM_TRY(in.upload(i_co, col_off, s));
    SFM_TRY(tm.mark(s));

    const unsigned gy = (unsigned)(P < 65535 ? P : 65535);
    const uint8_t *d_desc = in.ptr(i_desc);
    const int64_t *d_is = in.ptr(i_is), *d_ro = in.ptr(i_ro), *d_co = in.ptr(i_co);
    const int32_t *d_pairs = in.ptr(i_pairs);
    int32_t *d_norm = work.ptr(w_norm);
    int32_t *d_nn = out.ptr(o_nn), *d_d1 = out.ptr(o_d1), *d_d2 = out.ptr(o_d2);
    int32_t *d_rev = reverse ? out.ptr(o_rev) : nullptr;
    if (n_kp > 0) {
        const dim3 g_norm((unsigned)ceil_div(n_kp * (dim / 16), MD_THREADS));
#define MD_NORMS(D) MD_LAUNCH(k_md_norms<D>, g_norm, d_desc, n_kp, d_norm)
        MD_BY_DIM(MD_NORMS);
#undef MD_NORMS
    }
    if (max_i > 0) {
        const dim3 g_fwd((unsigned)ceil_div(max_i, MD_BM), gy);
#define MD_FWD(D) MD_LAUNCH((k_md_nn<D, false>), g_fwd, d_desc, d_norm, d_is, d_pairs, P, d_ro, d_nn, d_d1, d_d2)
        MD_BY_DIM(MD_FWD);
#undef MD_FWD
    }
    if (reverse && max_j > 0) {
        const dim3 g_rev((unsigned)ceil_div(max_j, MD_BM), gy);
#define MD_REV(D)                                                                                    \
    MD_LAUNCH((k_md_nn<D, true>), g_rev, d_desc, d_norm, d_is, d_pairs, P, d_co, d_rev, (int32_t *)nullptr, \
              (int32_t *)nullptr)
        MD_BY_DIM(MD_REV);
#undef MD_REV
    }
    SFM_TRY(md_compact(s, P, max_i, n_rows, d_is, d_pairs, d_ro, d_co, d_nn, d_d1, d_d2,
                       cross_check ? (const int32_t *)d_rev : (const int32_t *)nullptr, ratio_sq, max_dsq,
                       work.ptr(w_flag), work.ptr(w_place), work.ptr(w_tmp), tmp_bytes, out.ptr(o_ms), out.ptr(o_a),
                       out.ptr(o_b), out.ptr(o_dsq)));
    SFM_TRY(tm.mark(s));

    // match_start first: its last entry sizes the other copies
    SFM_TRY(out.download(match_start, o_ms, s));
    SFM_HIP(hipStreamSynchronize(s));
    const size_t total = (size_t)match_start[P];
    SFM_TRY(out.download(match_a, o_a, 0, total, s));
    SFM_TRY(out.download(match_b, o_b, 0, total, s));
    SFM_TRY(out.download(match_dsq, o_dsq, 0, total, s));
    SFM_TRY(out.download(nn, o_nn, s));
    SFM_TRY(out.download(d1, o_d1, s));
    SFM_TRY(out.download(d2, o_d2, s));
    SFM_TRY(out.download(nn_rev, o_rev, s));
    SFM_TRY(tm.finish(s));
    return 0;
}
