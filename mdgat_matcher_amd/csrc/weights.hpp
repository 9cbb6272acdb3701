// The device copies of a checkpoint: one description of the weight images (WeightImages) and the views the forward's stages ask for.
#pragma once
#include <vector>
#include "layer_image.hpp"
#include "f64.hpp"

constexpr size_t NO_IMAGE = ~(size_t)0;
struct WeightMat {           // one matrix of the checkpoint: where it is in the blob and where its images are (NO_IMAGE: it has none)
    size_t w, b;             // blob offsets of the [rows][K] matrix and of its bias
    int rows, K;
    int pitch, nperm, kpad;  // row image: row pitch (halves); the first nperm rows in the P/Q row order of layer.hip; kpad != 0: the
                             // planes zero-padded to kpad columns (launch_split_rows_pad) instead of [hi K | lo K | pad]
    size_t row, frag, frag64;  // halves into the split buffer: row image, f16 fragment image; doubles into the fp64 fragment buffer
};
enum { MAT_W1, MAT_W2, MAT_QKV };                               // the matrices of a layer: mlp.0 | mlp.3 | q|k|v
enum { ENC_K0, ENC_D0, ENC_K1, ENC_K2, ENC_D1, ENC_L };         // the encoders': kenc.0 | denc.0 | kenc.3 | kenc.6 | denc.3 | last convs summed

struct WeightImages {
    int L2;                       // propagation layers
    std::vector<WeightMat> mats;  // in blob order: the 2L layers' three, final_proj, the encoders' six
    size_t halves, doubles;       // sizes of the split buffer and of the fp64 fragment buffer
    const WeightMat& layer(int i, int which) const { return mats[3 * i + which]; }
    const WeightMat& proj(int j) const { return mats[j < L2 ? 3 * j + MAT_QKV : 3 * L2]; }   // layer j's q|k|v; j == 2L: final_proj
    const WeightMat& enc(int e) const { return mats[3 * L2 + 1 + e]; }
};

// Three images, each filled matrix by matrix at a running offset:
//  * the split buffer (zero filled by mdgat_create) starts with the ROW images of layer.hip and encoder.hip: per layer
//    [w1 256 rows x ROWH256 | w2 128 x ROWH256 | qkv 384 x ROWH128] (row = hi plane | lo plane | 32 B pad; output rows in the P/Q
//    order of layer.hip except the v rows), then final_proj 128 x ROWH128 - the stage copies of layer.hip read whole KB, up to
//    512 B past a K = 256 block, hence the slack behind it - then the encoder's [kenc.3 64x2x32 | kenc.6 128x2x64 | denc.0 64x2x48 |
//    denc.3 128x2x64 | last convs 128x2x256] (kenc.0 is read from the blob);
//  * behind them the layers' and final_proj's matrices once more in FRAGMENT order for layer_split.hip, whose waves load their slice
//    of the weights straight into registers: [row block of 16][k-step of 32][plane hi / lo][lane (row l15, column g)] x 16 B, so that
//    a wave's load instruction reads one contiguous KB (launch_frag_image; no pads);
//  * the fp64 fragment buffer (exact mode, layer_f64.hip: launch_frag64): per layer w1 | w2 | qkv, then the encoders' six in blob order.
inline WeightImages mdgat_weight_images(const BlobLayout& bl, int L) {
    WeightImages im{2 * L, {}, 0, 0};
    auto mat = [&](size_t w, size_t b, int rows, int K) { im.mats.push_back(WeightMat{w, b, rows, K, 0, 0, 0, NO_IMAGE, NO_IMAGE, NO_IMAGE}); };
    for (size_t i = 0, lo = bl.layer0; i < 2 * (size_t)L; ++i, lo += bl.layer_stride) {
        mat(lo + bl.mlp1_w, lo + bl.mlp1_b, 256, 256);  mat(lo + bl.mlp2_w, lo + bl.mlp2_b, 128, 256);  mat(lo + bl.qkv_w, lo + bl.qkv_b, 384, 128);
    }
    mat(bl.final_w, bl.final_b, 128, 128);
    mat(bl.kenc0_w, bl.kenc0_b, 32, 4);    mat(bl.denc0_w, bl.denc0_b, 64, 33);   mat(bl.kenc1_w, bl.kenc1_b, 64, 32);
    mat(bl.kenc2_w, bl.kenc2_b, 128, 64);  mat(bl.denc1_w, bl.denc1_b, 128, 64);  mat(bl.encl_w, bl.encl_b, 128, 256);
    WeightMat *const m = im.mats.data(), *const fin = m + 6 * L, *const enc = fin + 1;
    auto row = [&](WeightMat& t, int pitch, int nperm, int kpad = 0, size_t slack = 0) {
        t.pitch = pitch; t.nperm = nperm; t.kpad = kpad; t.row = im.halves; im.halves += (size_t)t.rows * pitch + slack;
    };
    for (WeightMat* l = m; l < fin; l += 3) { row(l[MAT_W1], ROWH256, 256); row(l[MAT_W2], ROWH256, 128); row(l[MAT_QKV], ROWH128, 256); }
    row(*fin, ROWH128, 128, 0, 512);
    row(enc[ENC_K1], 64, 0); row(enc[ENC_K2], 128, 0); row(enc[ENC_D0], 96, 0, 48); row(enc[ENC_D1], 128, 0); row(enc[ENC_L], 512, 0);
    for (WeightMat* t = m; t <= fin; ++t) { t->frag = im.halves; im.halves += (size_t)t->rows * 2 * t->K; }
    for (WeightMat& t : im.mats)
        if (&t != fin) { t.frag64 = im.doubles; im.doubles += frag64_doubles(t.rows, t.K); }
    return im;
}

struct Mat64 { const double *wf, *b; };   // an fp64 matrix in fragment order and its bias (LayerF64Args, EncoderF64Args)
// The five device copies of a handle's checkpoint and what the stages read of them.  No ownership: mdgat_create / mdgat_destroy.
struct DeviceWeights {
    BlobLayout bl{};
    WeightImages im{};
    float* blob = nullptr;      // fp32 blob (pack.py layout)
    _Float16* split = nullptr;  // row images (layer.hip, encoder.hip) and f16 fragment images (layer_split.hip)
    double* blob64 = nullptr;   // MDGAT_ARITH_FP64: the blob in fp64 (f64.hip), else nullptr
    double* frag64 = nullptr;   // MDGAT_ARITH_FP64: fp64 fragment images (layer_f64.hip), else nullptr
    Layer32 layer32(int i) const {
        const WeightMat &a = im.layer(i, MAT_W1), &c = im.layer(i, MAT_W2);
        return {split + a.row, split + c.row, split + a.frag, split + c.frag, blob + a.b, blob + c.b};
    }
    Proj32 proj32(int j) const { const WeightMat& t = im.proj(j); return {split + t.row, split + t.frag, blob + t.b, j < im.L2 ? 1 : 2}; }
    Encoder32 encoder32() const {
        return {blob, bl.kenc0_w, bl.kenc0_b, bl.denc0_b, bl.kenc1_b, bl.kenc2_b, bl.denc1_b, bl.encl_b, split + im.enc(ENC_K1).row,
                split + im.enc(ENC_K2).row, split + im.enc(ENC_D0).row, split + im.enc(ENC_D1).row, split + im.enc(ENC_L).row};
    }
    Mat64 mat64(const WeightMat* m) const { return m ? Mat64{frag64 + m->frag64, blob64 + m->b} : Mat64{nullptr, nullptr}; }   // null: no such product
};
