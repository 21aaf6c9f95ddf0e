// Sanitizer driver for the HOST side of libgpp_hip (make asan; tests/test_host_fuzz.py).  Test infrastructure, not part of the library.
//
// Every C-ABI entry point validates its descriptors on the host before anything reaches the device; the device-free ones -- gpp_conv2d_flops,
// gpp_conv2d_split_rule, gpp_conv2d_workspace_bytes, gpp_conv2d_tile_candidates, gpp_stem_pack_weights_f16 / _f16x3 -- and the argument checks of
// the launching ones (gpp_conv2d_igemm, gpp_bottleneck_tail, gpp_bottleneck_block, gpp_plan_run, gpp_poll_f32, gpp_draw_build, gpp_draw_raster, gpp_poll_costs_u16, gpp_plane_select, gpp_pose_costs_u16, gpp_plane_select_polled, gpp_road_*, ...: without a device they end
// in an error code before any launch) are run here over a file of descriptors the test generated, in a build of the library's host code
// with -fsanitize=address,undefined.  A bad descriptor must come back as GPP_ERR_* (or a hipError_t from the absent device); nothing may
// trip a sanitizer.  Device pointers inside the descriptors are never dereferenced by host code: they are fuzzed like every other field.
//
// File format: repeated records  [uint32 kind][uint32 a][uint32 b][uint32 c][gpp_conv_desc x 3]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime_api.h>

#include "gpp.h"

static long g_rc_hist[3] = {0, 0, 0};      // GPP_OK, GPP_ERR_*, hipError_t

static void note(int rc)
{
    if (rc == 0) ++g_rc_hist[0];
    else if (rc < 0 && rc >= -4) ++g_rc_hist[1];
    else if (rc > 0) ++g_rc_hist[2];
    else { fprintf(stderr, "unexpected return code %d\n", rc); exit(3); }
}

struct Rec { uint32_t kind, a, b, c; gpp_conv_desc d[3]; };

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s records.bin  (record = %zu bytes, gpp_conv_desc = %zu)\n", argv[0], sizeof(Rec), sizeof(gpp_conv_desc)); return 2; }
    if (!strcmp(argv[1], "--sizes")) { printf("%zu %zu\n", sizeof(Rec), sizeof(gpp_conv_desc)); return 0; }
    // a descriptor that passes every check is LAUNCHED where a device is visible -- on fuzzed pointers: this driver is for machines without one
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) {
        fprintf(stderr, "%d HIP device(s) visible: run with HIP_VISIBLE_DEVICES=-1 ROCR_VISIBLE_DEVICES= (tests/test_host_fuzz.py does)\n", devices);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror("open"); return 2; }
    Rec r;
    long n = 0;
    while (fread(&r, sizeof r, 1, f) == 1) {
        ++n;
        double flops = 0;
        int split = 0, count = 0;
        size_t bytes = 0;
        note(gpp_conv2d_flops(&r.d[0], &flops));
        note(gpp_conv2d_split_rule(&r.d[0], &split));
        note(gpp_conv2d_workspace_bytes(&r.d[0], &bytes));
        {
            const int cap = (int)(r.a % 80);
            std::vector<int> tiles((size_t)cap + 1);      // exactly `cap` usable entries + a canary the library must not touch
            tiles[cap] = 0x5a5a5a5a;
            note(gpp_conv2d_tile_candidates(&r.d[0], tiles.data(), cap, &count));
            if (tiles[cap] != 0x5a5a5a5a) { fprintf(stderr, "tile_candidates wrote past its capacity\n"); return 3; }
        }
        note(gpp_conv2d_flops(nullptr, &flops));
        note(gpp_conv2d_tile_candidates(&r.d[0], nullptr, 0, &count));
        switch (r.kind % 6) {
        case 0: {
            note(gpp_conv2d_igemm(&r.d[0], nullptr));
            // the same layer as one of both forms on the deep lists (fields of the neighbouring records stand in for the lists), and with
            // a lists_after handle: nobody has registered one here, so every value but 0 must come back as an error before any launch
            gpp_conv_desc v = r.d[0];
            v.deep_rows = r.d[1].tower_rows ? r.d[1].tower_rows : (const int32_t*)r.d[1].out;
            v.deep_counts = (r.b & 1) ? (const int32_t*)r.d[1].bias : r.d[1].tower_counts;
            v.deep_flag = (r.b & 2) ? (const int32_t*)r.d[2].out : r.d[2].tower_flag;
            v.deep_tile = (r.b & 4) ? 0 : (r.b & 8) ? 8000256 : (int32_t)r.c;
            if (r.b & 16) v.tower_rows = v.tower_counts = v.tower_flag = nullptr;
            if (r.b & 32) { v.gather_rows = nullptr; v.gather_counts = nullptr; v.guard = nullptr; }
            note(gpp_conv2d_igemm(&v, nullptr));
            v = r.d[0];
            v.lists_after = (int32_t)(r.c % 5) - 1;
            const int rc = gpp_conv2d_igemm(&v, nullptr);
            if (v.lists_after != 0 && rc == 0) { fprintf(stderr, "a lists_after handle nobody holds was accepted\n"); return 3; }
            note(rc);
            // conv_after and its registry: a handle nobody holds is refused like the other one; a descriptor is kept only when it passes
            // gpp_conv2d_igemm's checks as a layer of both forms that names nothing behind itself, and its handle then passes those of
            // the layer that carries it (run with check_only: nothing of it is launched)
            v = r.d[0];
            v.conv_after = (int32_t)(r.a % 5) - 1;
            v.conv_before = (r.b & 64) ? (int32_t)(r.c % 7) - 2 : 0;
            const int rc_after = gpp_conv2d_igemm(&v, nullptr);
            if ((v.conv_after != 0 || v.conv_before != 0) && rc_after == 0) { fprintf(stderr, "a conv_after handle nobody holds was accepted\n"); return 3; }
            note(rc_after);
            gpp_conv_desc w = r.d[1];
            if (r.b & 128) { w.deep_rows = (const int32_t*)r.d[2].out; w.deep_counts = (const int32_t*)r.d[2].bias; w.deep_flag = (const int32_t*)r.d[2].zero_page; }
            if (r.b & 256) { w.lists_after = 0; w.conv_after = 0; w.conv_before = 0; }
            int32_t held = 0;
            const int rc_reg = gpp_conv2d_deferred_register(&w, &held);
            note(rc_reg);
            note(gpp_conv2d_deferred_register(&w, nullptr));
            note(gpp_conv2d_deferred_register(nullptr, &held));
            note(gpp_conv2d_deferred_run((int32_t)r.c, 1, nullptr));
            if (rc_reg == 0) {
                if (!w.deep_rows || w.lists_after || w.conv_after || w.conv_before) { fprintf(stderr, "a deferred layer that is no end of a chain was kept\n"); return 3; }
                note(gpp_conv2d_deferred_run(held, 1, nullptr));
                v = r.d[0];
                v.conv_after = held;
                note(gpp_conv2d_igemm(&v, nullptr));
                v.conv_after = 0;
                v.conv_before = held;      // the same layer in front of a plain call: dense, its lists dropped (no device here: an error code either way)
                note(gpp_conv2d_igemm(&v, nullptr));
                v.conv_after = held;
                note(gpp_conv2d_deferred_release(held));
                v.gather_rows = nullptr; v.gather_counts = nullptr; v.guard = nullptr;
                const int rc_gone = gpp_conv2d_igemm(&v, nullptr);
                if (rc_gone == 0) { fprintf(stderr, "a released conv_after handle was accepted\n"); return 3; }
                note(rc_gone);
            }
            note(gpp_conv2d_deferred_release(held));
            note(gpp_conv2d_deferred_release((int32_t)r.b));
            break;
        }
        case 1: note(gpp_bottleneck_tail(&r.d[0], &r.d[1], (int)(r.b % 200), nullptr)); break;
        case 2:
            note(gpp_bottleneck_block(&r.d[0], &r.d[1], &r.d[2], (int)(r.b % 2000), nullptr));
            note(gpp_bottleneck_block_proj(&r.d[0], &r.d[1], &r.d[2], (r.c & 1) ? &r.d[r.c % 3] : nullptr, (int)(r.b % 2000), nullptr));
            break;
        case 3: {
            // a plan of a few ops over these descriptors (kinds and lane / join / sync flags fuzzed)
            gpp_tail_desc t = {&r.d[0], &r.d[1], (int32_t)(r.b % 200), 0};
            // (form 1, now and then 2: the record with the projection layer behind it)
            gpp_block_proj_desc bl = {{&r.d[0], &r.d[1], &r.d[2], (int32_t)(r.c % 2000), (int32_t)((r.c >> 11) % 3)}, &r.d[(r.c >> 13) % 3]};
            // (a kind whose descriptor type the record does not carry gets a conv descriptor's bytes, or NULL: every entry point checks its own
            // arguments, and none of the other descriptor types is larger than a gpp_conv_desc)
            static_assert(sizeof(gpp_conv_desc) >= sizeof(gpp_detect_desc) && sizeof(gpp_conv_desc) >= sizeof(gpp_poll_desc) &&
                          sizeof(gpp_conv_desc) >= sizeof(gpp_stem_desc) && sizeof(gpp_conv_desc) >= sizeof(gpp_relu_desc) &&
                          sizeof(gpp_conv_desc) >= sizeof(gpp_pool_desc), "the stand-in bytes cover every descriptor type");
            gpp_plan_op ops[4];
            for (int i = 0; i < 4; ++i) {
                const uint32_t k = (r.a >> (8 * i)) & 0xff;
                ops[i].kind = (int32_t)((k % 3 == 0) ? GPP_OP_CONV : (k % 3 == 1) ? GPP_OP_BOTTLENECK_TAIL : GPP_OP_BOTTLENECK_BLOCK);
                if (((r.c >> (3 * i)) & 7) == 7) ops[i].kind = (int32_t)((r.c >> 3) & 0x1f);      // now and then: any kind at all
                const int kk = ops[i].kind & 0xff;
                if (k & 0x40) ops[i].kind |= GPP_OP_LANE((k >> 4) & 3);
                if (k & 0x80) ops[i].kind |= GPP_OP_JOIN;
                if ((r.b >> i) & 1) ops[i].kind |= GPP_OP_SYNC;
                ops[i].tag = (int32_t)(k & 1);
                ops[i].desc = kk == GPP_OP_CONV ? (const void*)&r.d[i % 3]
                            : kk == GPP_OP_BOTTLENECK_TAIL ? (const void*)&t
                            : kk == GPP_OP_BOTTLENECK_BLOCK ? (const void*)&bl : (((r.b >> (4 + i)) & 1) ? (const void*)&r.d[0] : nullptr);
            }
            note(gpp_plan_run(ops, (int)(r.b % 5), nullptr, nullptr, 0));
            note(gpp_plan_run(nullptr, 1, nullptr, nullptr, 0));
            note(gpp_plan_run(ops, -1, nullptr, nullptr, 0));
            break;
        }
        case 4: {
            // host-side weight packers: source [147][64] float32, destination of a fuzzed size
            std::vector<float> src(147 * 64);
            for (size_t i = 0; i < src.size(); ++i) src[i] = (float)((int)((r.a + 2654435761u * i) % 2001) - 1000) * ((r.b & 1) ? 1e-3f : 1e30f);
            const size_t need16 = 64 * 232 * 2, need_x3 = 2 * 64 * 232 * 2 + 64 * 4;
            const size_t sz = (r.c % 3 == 0) ? need16 : (r.c % 3 == 1) ? need_x3 : (size_t)(r.c % 70000);
            std::vector<unsigned char> dst(sz ? sz : 1);
            note(gpp_stem_pack_weights_f16(src.data(), dst.data(), sz));
            note(gpp_stem_pack_weights_f16x3(src.data(), dst.data(), sz));
            note(gpp_stem_pack_weights_f16(nullptr, dst.data(), sz));
            break;
        }
        default: {
            size_t wb = 0;
            note(gpp_poll_workspace_bytes((int)r.a, (int)r.b, (int)(r.c & 1), &wb));
            note(gpp_detect_workspace_bytes((int)r.a, (int64_t)(((uint64_t)r.b * (uint64_t)r.c) >> ((r.a >> 8) & 31)), &wb));
            note(gpp_detect_osf_workspace_bytes((int)r.a, (int64_t)(((uint64_t)r.b * (uint64_t)r.c) >> ((r.a >> 8) & 31)), &wb));
            {
                // gpp_detect_deep_lists and its registry: a descriptor out of the record's bytes (checked on the host, launched nowhere here)
                static_assert(sizeof(gpp_conv_desc) >= sizeof(gpp_deep_list_desc), "the record's bytes cover a deep-list descriptor");
                gpp_deep_list_desc dl;
                memcpy(&dl, &r.d[1], sizeof dl);
                note(gpp_detect_deep_lists(&dl, nullptr));
                dl.reserved = 0; dl.B = (int32_t)(r.a % 9); dl.n_levels = (int32_t)(r.b % 7); dl.num_base_anchors = (int32_t)(r.c % 14);
                dl.max_rows = (int32_t)(r.a >> 8); dl.tower_max_rows = (int32_t)(r.b >> 8); dl.deep_max_rows = (int32_t)(r.c >> 8);
                int64_t pixels = 0;
                for (int l = 0; l < GPP_MAX_GROUPS; ++l) {
                    dl.level_width[l] = (int32_t)((r.a >> (3 * l)) % 40) + ((r.b >> l) & 1);
                    dl.level_pixels[l] = dl.level_width[l] * (int32_t)((r.c >> (3 * l)) % 30);
                    if (l < dl.n_levels) pixels += dl.level_pixels[l];
                }
                dl.n_anchors = (r.a & 64) ? (int64_t)r.b : pixels * dl.num_base_anchors;
                // layer 0's lists: none of the five fields, all of them (aligned), or whatever the record holds -- all or none, never without layer 1's
                if (r.a & 128) dl.radius4 = nullptr, dl.rows0 = dl.counts0 = dl.flag0 = dl.stats0 = nullptr;
                else if (r.a & 256) dl.radius4 = dl.marks, dl.rows0 = dl.rows2, dl.counts0 = dl.counts2, dl.flag0 = dl.flag2, dl.stats0 = dl.stats;
                if (r.a & 512) dl.rows1 = nullptr;
                note(gpp_detect_deep_lists(&dl, nullptr));
                note(gpp_detect_deep_lists(nullptr, nullptr));
                int32_t handle = 0;
                const int rc = gpp_detect_deep_lists_register(&dl, &handle);
                note(rc);
                note(gpp_detect_deep_lists_register(&dl, nullptr));
                note(gpp_detect_deep_lists_run((int32_t)r.c, 1, nullptr));
                if (rc == 0) {
                    note(gpp_detect_deep_lists_run(handle, 1, nullptr));
                    note(gpp_detect_deep_lists_release(handle));
                }
                note(gpp_detect_deep_lists_release(handle));
                note(gpp_detect_deep_lists_release((int32_t)r.b));
            }
            note(gpp_poll_f32(nullptr, nullptr, nullptr, nullptr, nullptr, (int)r.a, (int)r.b, (int)r.c, 0, 0.7f, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
            // the composite's host halves: sizes, then argument checks that end before any launch (fuzzed, misaligned and null pointers)
            size_t pb = 0;
            note(gpp_draw_workspace_bytes((int)r.a, (int)r.b, &pb, &wb));
            note(gpp_draw_workspace_bytes((int)(r.a % 64), (int)(r.b % 2000), &pb, nullptr));
            note(gpp_draw_build(nullptr, nullptr, (int)r.a, (int)r.b, 0.4f, nullptr, nullptr, nullptr));
            note(gpp_draw_build((const float*)r.d[0].in, (const double*)((uintptr_t)r.d[0].weight | 4), (int)(r.a % 64) + 1, (int)(r.b % 200) + 1, 0.4f,
                                r.d[0].out, (int32_t*)(uintptr_t)r.d[0].bias, nullptr));
            note(gpp_draw_raster(nullptr, nullptr, (int)r.a, (int)r.b, nullptr, nullptr, (int)r.c, nullptr, nullptr, nullptr));
            note(gpp_draw_raster((const uint8_t*)r.d[0].in, (const int32_t*)(uintptr_t)r.d[0].bias, (int)(r.a % 3000) + 1, (int)(r.b % 3000) + 1,
                                 (const void*)((uintptr_t)r.d[0].weight | 8), (const int32_t*)(uintptr_t)r.d[0].bias, (int)(r.c % 64) + 1, (uint8_t*)r.d[0].out,
                                 r.d[0].out, nullptr));
            // the cuboid NMS: null pointers, more rows than the kept mask holds, a threshold outside (0, 1) -- all end before any launch
            note(gpp_cuboid_nms_f64(nullptr, (int)r.a, (int)r.b, (int)(r.c % 4), 0.3, nullptr, nullptr, nullptr, nullptr));
            note(gpp_cuboid_nms_f64((const float*)r.d[0].in, (int)(r.a % 64) + 1, 129 + (int)(r.b % 2000), (int)(r.c & 1), 0.3, (float*)r.d[0].out,
                                    (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias, nullptr));
            note(gpp_cuboid_nms_f64((const float*)r.d[0].in, (int)(r.a % 64) + 1, (int)(r.b % 128) + 1, (int)(r.c & 1), (double)(r.c % 3) - 1.0, (float*)r.d[0].out,
                                    (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias, nullptr));
            // the tracker: sizes, then fuzzed parameters and sequence starts against null pointers, more rows than a workgroup has threads, and a
            // workspace of no bytes -- all end before any launch or copy (seq_start is the one host array the call reads)
            {
                gpp_track_params tp = {(int32_t)(r.c % 5) - 1, (int32_t)(r.a % 7) - 2, (int32_t)(r.b % 3), (int32_t)(r.c % 11 == 0),
                                       (double)(r.c % 7) * 0.5 - 0.5, (double)(r.a % 4) * 0.5, (double)(r.b % 4) * 0.5 - 0.5, 0.25, 0.0};
                int32_t seq[3] = {(int32_t)(r.c % 3) - 1, (int32_t)(r.a % 9), (int32_t)(r.b % 9)};
                size_t tb = 0;
                note(gpp_track_state_bytes(&tb));
                note(gpp_track_workspace_bytes((int)r.a, &tb));
                note(gpp_track_workspace_bytes((int)(r.a % 64), nullptr));
                note(gpp_track_f64(nullptr, (int)r.a, (int)r.b, seq, 2, nullptr, nullptr, &tp, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
                note(gpp_track_f64((const float*)r.d[0].in, 8, 129 + (int)(r.b % 2000), seq, 2, r.d[0].in, r.d[0].out, &tp, (float*)r.d[0].out,
                                   (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias, r.d[0].out, (size_t)r.d[0].partial_bytes, nullptr));
                note(gpp_track_f64((const float*)r.d[0].in, 8, (int)(r.b % 128) + 1, seq, 2, r.d[0].in, r.d[0].out, &tp, (float*)r.d[0].out,
                                   (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias, (void*)((uintptr_t)r.d[0].out | 8), 0, nullptr));
                // (the optimal assignment's entry point shares every check: the same three calls)
                note(gpp_track_optimal_f64(nullptr, (int)r.a, (int)r.b, seq, 2, nullptr, nullptr, &tp, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
                note(gpp_track_optimal_f64((const float*)r.d[0].in, 8, 129 + (int)(r.b % 2000), seq, 2, r.d[0].in, r.d[0].out, &tp, (float*)r.d[0].out,
                                           (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias, r.d[0].out, (size_t)r.d[0].partial_bytes,
                                           nullptr));
                note(gpp_track_optimal_f64((const float*)r.d[0].in, 8, (int)(r.b % 128) + 1, seq, 2, r.d[0].in, r.d[0].out, &tp, (float*)r.d[0].out,
                                           (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias, (void*)((uintptr_t)r.d[0].out | 8), 0,
                                           nullptr));
                // the ego records are the second host array a call reads: 8 of them (seq_start never passes 8 here), one word fuzzed to a
                // NaN, an infinity or a padding word that is not 0 -- the frames inside a sequence are read, and only those
                double ego[8 * GPP_TRACK_EGO_FIELDS] = {0.0};
                for (int f = 0; f < 8; ++f) ego[f * GPP_TRACK_EGO_FIELDS] = ego[f * GPP_TRACK_EGO_FIELDS + 4] = ego[f * GPP_TRACK_EGO_FIELDS + 8] = 1.0;
                const double odd[4] = {0.0, __builtin_nan(""), __builtin_inf(), 1.0};
                ego[(r.a % 8) * GPP_TRACK_EGO_FIELDS + r.b % GPP_TRACK_EGO_FIELDS] = odd[r.c % 4];
                note(gpp_track_ego_workspace_bytes((int)r.a, (int)r.b, &tb));
                note(gpp_track_ego_workspace_bytes((int)(r.a % 64), (int)(r.b % 64), nullptr));
                note(gpp_track_ego_f64(nullptr, 8, (int)r.b, seq, 2, nullptr, nullptr, &tp, ego, (int)(r.c % 4) - 1, nullptr, nullptr, nullptr, nullptr, 0,
                                       nullptr));
                note(gpp_track_ego_f64(nullptr, (int)r.a, (int)r.b, seq, 2, nullptr, nullptr, &tp, nullptr, (int)(r.c & 1), nullptr, nullptr, nullptr,
                                       nullptr, 0, nullptr));
                note(gpp_track_ego_f64((const float*)r.d[0].in, 8, (int)(r.b % 128) + 1, seq, 2, r.d[0].in, r.d[0].out, &tp, ego, (int)(r.c & 1),
                                       (float*)r.d[0].out, (int32_t*)(uintptr_t)r.d[0].bias, (int32_t*)(uintptr_t)r.d[0].bias,
                                       (void*)((uintptr_t)r.d[0].out | 8), 0, nullptr));
            }
            // the tracking score: fuzzed parameters, sizes and sequence starts against null pointers, more rows or trajectories than the kernels
            // take, and a workspace of no bytes -- all end before any launch or copy (seq_start is the one host array gpp_mot_clear reads)
            {
                gpp_mot_params mp = {(int32_t)(r.c % 5) - 1, (int32_t)(r.c % 11 == 0), (double)(r.a % 5) * 0.5 - 0.5, (double)(r.b % 4), 0.0, 25.0};
                int32_t seq[3] = {(int32_t)(r.c % 3) - 1, (int32_t)(r.a % 9), (int32_t)(r.b % 9)};
                size_t wb = 0;
                note(gpp_mot_clear_workspace_bytes((int)r.a, &wb));
                note(gpp_mot_clear_workspace_bytes((int)(r.a % 64), nullptr));
                note(gpp_mot_assign(nullptr, nullptr, nullptr, nullptr, nullptr, (int)r.a, (int)r.b, (int)r.c, &mp, nullptr, nullptr, nullptr, nullptr, nullptr));
                note(gpp_mot_assign((const double*)r.d[0].in, (const double*)r.d[0].in, (const int32_t*)(uintptr_t)r.d[0].bias, (const float*)r.d[0].in,
                                    (const int32_t*)(uintptr_t)r.d[0].bias, 8, 129 + (int)(r.b % 2000), (int)(r.c % 128), &mp, (int32_t*)r.d[0].out,
                                    (int32_t*)r.d[0].out, (int32_t*)r.d[0].out, (int64_t*)r.d[0].out, nullptr));
                note(gpp_mot_clear(nullptr, nullptr, nullptr, nullptr, nullptr, (int)r.a, (int)r.b, (int)r.c, seq, 2, (int)(r.b % 2048), nullptr, nullptr,
                                   nullptr, 0, nullptr));
                note(gpp_mot_clear((const int32_t*)r.d[0].in, (const int32_t*)r.d[0].in, (const int32_t*)r.d[0].in, (const int32_t*)r.d[0].in,
                                   (const int64_t*)r.d[0].in, 8, (int)(r.b % 128) + 1, (int)(r.c % 128) + 1, seq, 2, 1025 + (int)(r.a % 100),
                                   (int64_t*)r.d[0].out, (int32_t*)r.d[0].out, r.d[0].out, 0, nullptr));
                note(gpp_mot_clear((const int32_t*)r.d[0].in, (const int32_t*)r.d[0].in, (const int32_t*)r.d[0].in, (const int32_t*)r.d[0].in,
                                   (const int64_t*)r.d[0].in, 8, (int)(r.b % 128) + 1, (int)(r.c % 128) + 1, seq, 2, (int)(r.a % 1024),
                                   (int64_t*)r.d[0].out, (int32_t*)r.d[0].out, (void*)((uintptr_t)r.d[0].out | 2), 0, nullptr));
            }
            // the plane distillation's host halves: sizes, then argument checks (bad pitch, K > M, null and misaligned pointers) that end before any launch
            note(gpp_poll_costs_workspace_bytes((int)r.a, &wb));
            note(gpp_plane_select_workspace_bytes((int)r.b, nullptr));
            note(gpp_poll_costs_u16(nullptr, nullptr, nullptr, nullptr, nullptr, (int)r.a, (int)r.b, (int)r.c, 0.7f, nullptr, (int)(r.a * r.b), nullptr,
                                    (int64_t)r.c, (int64_t)(int32_t)r.b, nullptr, 0, nullptr));
            note(gpp_poll_costs_u16((const float*)r.d[0].in, (const float*)r.d[0].in, (const int32_t*)(uintptr_t)r.d[0].bias, (const float*)r.d[0].in,
                                    (const float*)((uintptr_t)r.d[0].weight | 4), (int)(r.a % 64) + 1, (int)(r.b % 64) + 1, (int)(r.c % 3000) + 1, 0.7f,
                                    (const int32_t*)(uintptr_t)r.d[0].bias, (int)(r.b % 500), (uint16_t*)r.d[0].out, (int64_t)((r.c % 3000) + 8) / 8 * 8, 0,
                                    r.d[0].out, (size_t)r.d[0].partial_bytes, nullptr));
            note(gpp_plane_select(nullptr, (int)r.a, (int)r.b, (int64_t)(int32_t)r.c, (int)r.c, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr));
            note(gpp_plane_select((const uint16_t*)((uintptr_t)r.d[0].in | 2), (int)(r.a % 5000) + 1, (int)(r.b % 3000) + 1, (int64_t)((r.b % 3000) + 8) / 8 * 8,
                                  (int)(r.c % 16) + 1, (int32_t*)(uintptr_t)r.d[0].bias, (uint64_t*)r.d[0].out, (uint16_t*)r.d[0].out,
                                  (int32_t*)(uintptr_t)r.d[0].bias, r.d[0].out, (size_t)r.d[0].partial_bytes, nullptr));
            // ... and of the polled-location pair (two tables: either one null or misaligned, a short workspace, K > M, a bad pitch)
            note(gpp_plane_select_polled_workspace_bytes((int)r.b, nullptr));
            note(gpp_plane_select_polled_workspace_bytes((int)r.a, &wb));
            note(gpp_pose_costs_u16(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, (int)r.a, (int)r.b, (int)r.c, 0.7f, nullptr, (int)(r.a * r.b),
                                    nullptr, nullptr, (int64_t)r.c, (int64_t)(int32_t)r.b, nullptr, 0, nullptr));
            note(gpp_pose_costs_u16((const float*)r.d[0].in, (const float*)r.d[0].in, (const int32_t*)(uintptr_t)r.d[0].bias, (const float*)r.d[0].in,
                                    (const float*)r.d[0].in, (const float*)((uintptr_t)r.d[0].weight | ((r.a & 1) ? 4 : 0)), (int)(r.a % 64) + 1,
                                    (int)(r.b % 64) + 1, (int)(r.c % 3000) + 1, 0.7f, (const int32_t*)(uintptr_t)r.d[0].bias, (int)(r.b % 500),
                                    (uint16_t*)r.d[0].out, (uint16_t*)((uintptr_t)r.d[0].out | ((r.a & 2) ? 2 : 0)), (int64_t)((r.c % 3000) + 8) / 8 * 8, 0,
                                    r.d[0].out, (size_t)r.d[0].partial_bytes, nullptr));
            note(gpp_pose_costs_u16((const float*)r.d[0].in, (const float*)r.d[0].in, (const int32_t*)(uintptr_t)r.d[0].bias, (const float*)r.d[0].in,
                                    (const float*)r.d[0].in, (const float*)r.d[0].weight, 2, 5, (int)(r.c % 3000) + 1, 0.7f, nullptr, 10,
                                    (uint16_t*)r.d[0].out, (r.a & 4) ? nullptr : (uint16_t*)r.d[0].out, (int64_t)(r.c % 3000) + 1, 0, r.d[0].out, 0, nullptr));
            note(gpp_plane_select_polled(nullptr, nullptr, (int)r.a, (int)r.b, (int64_t)(int32_t)r.c, (int)r.c, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, 0, nullptr));
            note(gpp_plane_select_polled((const uint16_t*)r.d[0].in, (const uint16_t*)((uintptr_t)r.d[0].in | 2), (int)(r.a % 5000) + 1, (int)(r.b % 3000) + 1,
                                         (int64_t)((r.b % 3000) + 8) / 8 * 8, (int)(r.c % 16) + 1, (int32_t*)(uintptr_t)r.d[0].bias, (uint64_t*)r.d[0].out,
                                         (uint16_t*)r.d[0].out, (uint16_t*)r.d[0].out, (int32_t*)(uintptr_t)r.d[0].bias, r.d[0].out,
                                         (size_t)r.d[0].partial_bytes, nullptr));
            note(gpp_plane_select_polled((const uint16_t*)r.d[0].in, (r.a & 1) ? nullptr : (const uint16_t*)r.d[0].in, 8, (int)(r.b % 64) + 1,
                                         (int64_t)(r.b % 64) + 1, (int)(r.c % 80), (int32_t*)(uintptr_t)r.d[0].bias, (uint64_t*)r.d[0].out, (uint16_t*)r.d[0].out,
                                         (uint16_t*)r.d[0].out, (int32_t*)(uintptr_t)r.d[0].bias, r.d[0].out, 0, nullptr));
            // the road fit's host halves: null pointers, F = 0, H = 0, region bounds over the caps, a frame bound above the total, NaN gates,
            // misaligned points and sums.  (The offsets are device memory: a descending pair is the kernels' to refuse, gpp.h.)
            {
                const int32_t* i32 = (const int32_t*)(uintptr_t)r.d[0].bias;
                const uint32_t* u32 = (const uint32_t*)(uintptr_t)r.d[0].bias;
                const int F = (int)(r.a % 70000), total = (int)(r.b >> 1), mp = (int)(r.c % ((1u << 20) + 3));
                const double nan = __builtin_nan(""), g = (r.a & 1) ? nan : (double)(int32_t)r.b;
                note(gpp_road_points_i32(nullptr, nullptr, nullptr, (int)r.a, (int)r.b, (int)r.c, 1, 1, 1, nullptr, nullptr, nullptr));
                note(gpp_road_points_i32(nullptr, nullptr, nullptr, 0, 0, 0, 5120, 2048, 12800, nullptr, nullptr, nullptr));
                note(gpp_road_points_i32((const float*)((uintptr_t)r.d[0].in | ((r.a & 2) ? 4 : 0)), i32, (const double*)r.d[0].weight, F, total, mp,
                                         (int)(r.a % 10243), (int)(r.b % 2051), (int)(r.c % 20483), (int32_t*)r.d[0].out, (int32_t*)r.d[0].out, nullptr));
                if (gpp_road_points_i32((const float*)r.d[0].in, i32, (const double*)r.d[0].weight, 1, 8, 8, 10240 + (r.a % 3 == 0), 2048 + (r.a % 3 == 1),
                                        20480 + (r.a % 3 == 2), (int32_t*)r.d[0].out, (int32_t*)r.d[0].out, nullptr) == 0) {
                    fprintf(stderr, "a road region over the caps was accepted\n"); return 3;
                }
                note(gpp_road_score(nullptr, nullptr, nullptr, nullptr, r.a, (int)r.b, (int)r.c, (int)r.a, (int)r.b, 0.9, 1.0, 2.0, 3.0, nullptr, nullptr));
                note(gpp_road_score(i32, i32, i32, u32, r.c, F, total, mp, 0, 0.9, 1.0, 2.0, 3.0, (int32_t*)r.d[0].out, nullptr));
                note(gpp_road_score(i32, i32, i32, u32, r.c, 0, total, 0, (int)(r.b % 5000), 0.9, 1.0, 2.0, 3.0, (int32_t*)r.d[0].out, nullptr));
                note(gpp_road_score(i32, i32, i32, u32, r.c, F, total, mp, (int)(r.b % 5000), g, g, (r.a & 4) ? nan : 2.0 * g, (double)(int32_t)r.c,
                                    (r.a & 8) ? nullptr : (int32_t*)r.d[0].out, nullptr));
                note(gpp_road_winner(nullptr, (int)r.a, (int)r.b, (int)r.c, nullptr, nullptr, nullptr));
                note(gpp_road_winner(i32, F, (int)(r.b % 5000), (int)(r.c % 300) - 1, (int32_t*)r.d[0].out, (r.a & 8) ? nullptr : (int32_t*)r.d[0].out, nullptr));
                note(gpp_road_moments(nullptr, nullptr, nullptr, nullptr, r.a, nullptr, (int)r.b, (int)r.c, (int)r.a, (int)r.b, 1.0, nullptr, nullptr));
                note(gpp_road_moments(i32, i32, i32, u32, r.c, i32, F, total, mp, (int)(r.b % 5000), (r.a & 4) ? nan : 655.36,
                                      (int64_t*)((uintptr_t)r.d[0].out | ((r.a & 16) ? 4 : 0)), nullptr));
                // the peel's host half: the workspace size over the whole range and beyond it, null pointers, F = 0, q_out == q_in and ranges
                // that overlap by one row, a workspace one byte short, misaligned buffers, a NaN threshold
                size_t peel = 0;
                note(gpp_road_peel_workspace_bytes((int)r.a, (int)r.b, (r.c & 1) ? nullptr : &peel));
                note(gpp_road_peel_workspace_bytes(F, mp, &peel));
                if (gpp_road_peel_workspace_bytes(F, mp, &peel) == 0 && peel < sizeof(int32_t) * (size_t)F * (size_t)((mp + 2047) / 2048)) {
                    fprintf(stderr, "a peel workspace smaller than its block counts\n"); return 3;
                }
                note(gpp_road_peel_i32(nullptr, nullptr, nullptr, nullptr, r.a, nullptr, (int)r.b, (int)r.c, (int)r.a, (int)r.b, 1.0, nullptr, nullptr,
                                       nullptr, 0, nullptr));
                note(gpp_road_peel_i32(i32, i32, i32, u32, r.c, i32, 0, total, 0, (int)(r.b % 5000), 1.0, (int32_t*)r.d[0].out, (int32_t*)r.d[0].out,
                                       r.d[0].out, 0, nullptr));
                int32_t* const qo = (int32_t*)((uintptr_t)r.d[0].out | ((r.a & 32) ? 2 : 0));
                note(gpp_road_peel_i32(i32, i32, i32, u32, r.c, i32, F, total, mp, (int)(r.b % 5000), (r.a & 4) ? nan : 655.36, qo, (int32_t*)r.d[0].out,
                                       (r.a & 64) ? nullptr : (void*)((uintptr_t)r.d[0].partial | ((r.a & 128) ? 1 : 0)),
                                       (r.a & 256) ? (peel ? peel - 1 : 0) : (size_t)r.d[0].partial_bytes, nullptr));
                if (F > 0 && total > 0 && mp <= total && i32 && (uintptr_t)i32 < ((uintptr_t)1 << 62)) {      // (no wrap-around of the fuzzed address)
                    const int32_t* const over = (r.a & 512) ? i32 : (const int32_t*)((uintptr_t)i32 + 12 * ((size_t)total - 1));
                    if (gpp_road_peel_i32(i32, i32, i32, u32, r.c, i32, F, total, mp, 8, 1.0, (int32_t*)(uintptr_t)over, (int32_t*)r.d[0].out,
                                          r.d[0].out, (size_t)-1, nullptr) != GPP_ERR_BAD_ARG) {
                        fprintf(stderr, "overlapping peel buffers were accepted\n"); return 3;
                    }
                }
            }
            break;
        }
        }
    }
    fclose(f);
    printf("%ld records: %ld GPP_OK, %ld GPP_ERR_*, %ld hipError_t\n", n, g_rc_hist[0], g_rc_hist[1], g_rc_hist[2]);
    return 0;
}
