// blob_layout.h — the canonical weight blob of include/kami_hip.h (kh_weight_count): every tensor's name (the reference's,
// nn.cpp:20-23,45-56), shape and float offset, in blob order.  The one C++ statement of that order: the blob parser, the
// checkpoint reader and writer and the trainer take their offsets from it (kami_amd/weights.py::tensor_specs is the
// Python one).  Plain C++17, host only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/kami_hip.h"

namespace kh_blob {

// shape: libtorch's (conv [Co][Ci][k][k], linear [out][in], bias / BatchNorm [Co]); at: float offset; n: elements
struct Tensor { std::string name; std::vector<int64_t> shape; size_t at, n; };

inline std::vector<Tensor> layout(int F, int C, int R)
{
    std::vector<Tensor> v;
    size_t at = 0;
    auto tensor = [&](const std::string& name, std::vector<int64_t> shape) {
        size_t n = 1;
        for (int64_t s : shape) n *= (size_t)s;
        v.push_back({ name, std::move(shape), at, n });
        at += n;
    };
    auto convbn = [&](const std::string& conv, const std::string& bn, int64_t co, int64_t ci, int64_t k) {
        tensor(conv + ".weight", { co, ci, k, k }); tensor(conv + ".bias", { co });
        for (const char* s : { ".weight", ".bias", ".running_mean", ".running_var" }) tensor(bn + s, { co });
    };
    convbn("conv1", "batchnorm1", C, F, 3);
    for (int i = 0; i < R; ++i) {
        const std::string r = "residual" + std::to_string(i);
        convbn(r + ".conv1", r + ".batchnorm1", C, C, 3);
        convbn(r + ".conv2", r + ".batchnorm2", C, C, 3);
    }
    convbn("policyconv", "pbatchnorm", KH_POLICY_MID, C, 1);
    tensor("policyconv2.weight", { KH_POLICY_PLANES, KH_POLICY_MID, 1, 1 }); tensor("policyconv2.bias", { KH_POLICY_PLANES });
    convbn("valueconv", "vbatchnorm", 1, C, 1);
    tensor("valuefc.weight", { KH_VALUE_WIDTH, 64 }); tensor("valuefc.bias", { KH_VALUE_WIDTH });
    return v;
}

inline size_t total(const std::vector<Tensor>& v) { return v.back().at + v.back().n; }      // floats in the blob

}  // namespace kh_blob
