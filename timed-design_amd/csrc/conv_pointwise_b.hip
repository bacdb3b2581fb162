// The chunk-blocked-output (BLK) and straight-line "BN-affine -> ReLU" epilogue (EPI = 2) instantiations of k_conv_pw2 — a second
// translation unit so that they compile next to conv_pointwise.hip's plain kernels, not after them.
#include "conv_pointwise_k.h"

namespace {
// chunk-blocked output, generic chain (no pooling): [kmax index][nt index], and the 12-slot pair
const PwEntry kPw2Blk[3][3] = {{PW2_ENTRY(4, 1, 0, 1, 0), PW2_ENTRY(4, 2, 0, 1, 0), PW2_ENTRY(4, 4, 0, 1, 0)},
                               {PW2_ENTRY(8, 1, 0, 1, 0), PW2_ENTRY(8, 2, 0, 1, 0), PW2_ENTRY(8, 4, 0, 1, 0)},
                               {PW2_ENTRY(16, 1, 0, 1, 0), PW2_ENTRY(16, 2, 0, 1, 0), PW_NONE}};
const PwEntry kPw2Blk_12[2] = {PW2_ENTRY(12, 1, 0, 1, 0), PW2_ENTRY(12, 2, 0, 1, 0)};
// "BN-affine -> ReLU" epilogue (EPI = 2), no pooling: [blk][kmax index][nt index], and the 12-slot pairs
// (up to 64 output / 96 input channels: the other shapes keep the generic chain)
const PwEntry kPw2Relu[2][3][3] = {{{PW2_ENTRY(4, 1, 0, 0, 2), PW2_ENTRY(4, 2, 0, 0, 2), PW_NONE},
                                    {PW2_ENTRY(8, 1, 0, 0, 2), PW2_ENTRY(8, 2, 0, 0, 2), PW_NONE},
                                    {PW_NONE, PW_NONE, PW_NONE}},
                                   {{PW2_ENTRY(4, 1, 0, 1, 2), PW2_ENTRY(4, 2, 0, 1, 2), PW_NONE},
                                    {PW2_ENTRY(8, 1, 0, 1, 2), PW2_ENTRY(8, 2, 0, 1, 2), PW_NONE},
                                    {PW_NONE, PW_NONE, PW_NONE}}};
const PwEntry kPw2Relu_12[2][2] = {{PW2_ENTRY(12, 1, 0, 0, 2), PW2_ENTRY(12, 2, 0, 0, 2)}, {PW2_ENTRY(12, 1, 0, 1, 2), PW2_ENTRY(12, 2, 0, 1, 2)}};
const PwEntry kPwNone = PW_NONE;
}  // namespace

const PwEntry* conv_pw2_extra(int blk, int epi, int kmi, int nti, int slot12) {
    if (blk < 0 || blk > 1 || kmi < 0 || kmi > 2 || nti < 0 || nti > 2) return &kPwNone;
    if (epi == 2) return slot12 ? (nti <= 1 ? &kPw2Relu_12[blk][nti] : &kPwNone) : &kPw2Relu[blk][kmi][nti];
    if (epi == 0 && blk == 1) return slot12 ? (nti <= 1 ? &kPw2Blk_12[nti] : &kPwNone) : &kPw2Blk[kmi][nti];
    return &kPwNone;
}

// the i-th entry of the three tables above and their 12-slot rows (entries without a kernel included), nullptr past the end
const PwEntry* conv_pw2_extra_at(int i) {
    if (i < 0) return nullptr;
    if (i < 9) return &kPw2Blk[i / 3][i % 3];
    if ((i -= 9) < 2) return &kPw2Blk_12[i];
    if ((i -= 2) < 18) return &kPw2Relu[i / 9][i / 3 % 3][i % 3];
    if ((i -= 18) < 4) return &kPw2Relu_12[i / 2][i % 2];
    return nullptr;
}
