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
//   k_md_nn      (in match_common.hpp, the one nearest-neighbour kernel: guided
//                matching instantiates it with its gate, retrieval.hip as here)
//                a workgroup of 4 waves owns md_bm = 128 rows of the pair's
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
    return md_run<MdNoGate>(desc, n_kp, img_start, n_images, dim, pairs, P, ratio, max_dsq, cross_check, capacity,
                            match_start, match_a, match_b, match_dsq, nn, d1, d2, nn_rev, MdGateIn(), device);
}
