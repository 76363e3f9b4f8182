// torch_archive_write.h — writes the checkpoints the reference's NN::write leaves on disk (kami/nn/nn.cpp:189-202):
//     serialize::OutputArchive a; mod->save(a); a.write("generation", IValue(generation)); a.save_to(path);
// so that a network trained by the engine loads in a stock kami (NN::read, nn.cpp:204-222) and in torch.jit.load.
// The layout is the one torch_archive.h reads back, reproduced from a reference checkpoint
// (tests/golden/ref_checkpoint_f30_c8_r1.pt):
//   <root>/data.pkl        protocol-2 pickle: one script-module object per module, tensors through
//                          torch._utils._rebuild_tensor_v2 over persistent ids ('storage', torch.<T>Storage, key, 'cpu', numel)
//   <root>/data/<key>      the tensor bytes, one record per tensor, key = 0, 1, 2, ... in pickling order
//   <root>/code/__torch__.py   the module classes: __parameters__, __buffers__ and the typed attributes
//   <root>/constants.pkl   an empty tuple;  <root>/version "3\n";  <root>/byteorder "little"
// All members are STORED (method 0) with their CRC-32; every member's bytes start on a 64-byte boundary (padding in
// the local header's extra field, as libtorch's writer does).  The .debug_pkl members and .data/serialization_id that
// libtorch also writes are left out: its loader does not need them.  No zip64: an archive that would need it is refused
// (the largest configured network, 20x256, is ~96 MB).  Plain C++17, host only, no libtorch.
#pragma once

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "blob_layout.h"

namespace kh_archive {

// a request the format cannot hold (zip64 size, bad shape): the caller's fault, not the file system's
struct Unsupported : std::runtime_error { using std::runtime_error::runtime_error; };

namespace wdetail {

inline uint32_t crc32(const uint8_t* p, size_t n, uint32_t crc = 0)
{
    static uint32_t table[256];
    static const bool init = [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = c & 1 ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        return true;
    }();
    (void)init;
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}

inline void put16(std::vector<uint8_t>& o, uint32_t v) { o.push_back((uint8_t)v); o.push_back((uint8_t)(v >> 8)); }
inline void put32(std::vector<uint8_t>& o, uint32_t v) { put16(o, v & 0xffff); put16(o, v >> 16); }

// ---- the pickle: only the opcodes torch_archive.h's reader (and libtorch's unpickler) take; no memo
struct Pickler {
    std::vector<uint8_t> b;
    void op(uint8_t c) { b.push_back(c); }
    void str(const std::string& s) { op(0x58); put32(b, (uint32_t)s.size()); b.insert(b.end(), s.begin(), s.end()); }   // BINUNICODE
    void global(const char* mod, const char* name)                                                                     // GLOBAL
    {
        op(0x63);
        b.insert(b.end(), mod, mod + strlen(mod)); b.push_back('\n');
        b.insert(b.end(), name, name + strlen(name)); b.push_back('\n');
    }
    void integer(int64_t v)
    {
        if (v >= 0 && v < 256) { op(0x4b); b.push_back((uint8_t)v); }                                                 // BININT1
        else if (v >= 0 && v < 65536) { op(0x4d); put16(b, (uint32_t)v); }                                             // BININT2
        else if (v >= INT32_MIN && v <= INT32_MAX) { op(0x4a); put32(b, (uint32_t)(int32_t)v); }                       // BININT
        else { op(0x8a); b.push_back(8); for (int k = 0; k < 8; ++k) b.push_back((uint8_t)((uint64_t)v >> (8 * k))); }  // LONG1
    }
    void ints(const std::vector<int64_t>& v) { op(0x28); for (int64_t x : v) integer(x); op(0x74); }                 // MARK ... TUPLE
    // _rebuild_tensor_v2(storage, 0, size, stride, requires_grad, OrderedDict())
    void tensor(const char* storage_type, const std::string& key, int64_t numel, const std::vector<int64_t>& shape, bool requires_grad)
    {
        global("torch._utils", "_rebuild_tensor_v2");
        op(0x28);
        op(0x28); str("storage"); global("torch", storage_type); str(key); str("cpu"); integer(numel); op(0x74); op(0x51);  // BINPERSID
        integer(0);
        ints(shape);
        std::vector<int64_t> stride(shape.size());
        int64_t s = 1;
        for (size_t k = shape.size(); k-- > 0;) { stride[k] = s; s *= shape[k]; }
        ints(stride);
        op(requires_grad ? 0x88 : 0x89);
        global("collections", "OrderedDict"); op(0x29); op(0x52);
        op(0x74); op(0x52);
    }
    void begin_object(const char* cls) { global("__torch__", cls); op(0x29); op(0x81); op(0x7d); op(0x28); }  // NEWOBJ, {} MARK
    void end_object() { op(0x75); op(0x62); }                                                                  // SETITEMS BUILD
};

struct Record { std::string name; const uint8_t* data; size_t size; };

// the zip container; throws Unsupported when zip64 would be needed, runtime_error on I/O failure
inline void write_zip(FILE* f, const std::vector<Record>& recs)
{
    constexpr uint64_t LIMIT = 0xffffffffull;
    if (recs.size() >= 0xffff) throw Unsupported("too many archive members (zip64 is not written)");
    uint64_t off = 0;
    std::vector<uint8_t> cd;
    auto out = [&](const void* p, size_t n) {
        if (n && fwrite(p, 1, n, f) != n) throw std::runtime_error(std::string("write failed: ") + strerror(errno));
        off += n;
    };
    for (const Record& r : recs) {
        const size_t nl = r.name.size();
        size_t pad = (64 - (off + 30 + nl) % 64) % 64;         // the member's bytes on a 64-byte boundary
        if (pad && pad < 4) pad += 64;                         // (an extra field is at least its 4-byte header)
        if (off > LIMIT || r.size > LIMIT || off + 30 + nl + pad + r.size > LIMIT)
            throw Unsupported("archive larger than 4 GiB (zip64 is not written)");
        const uint32_t crc = crc32(r.data, r.size), lho = (uint32_t)off;
        std::vector<uint8_t> h;
        put32(h, 0x04034b50); put16(h, 20); put16(h, 0); put16(h, 0); put16(h, 0); put16(h, 0x21);   // version, flags, STORED, 1980-01-01
        put32(h, crc); put32(h, (uint32_t)r.size); put32(h, (uint32_t)r.size);
        put16(h, (uint32_t)nl); put16(h, (uint32_t)pad);
        h.insert(h.end(), r.name.begin(), r.name.end());
        if (pad) { put16(h, 0x4246 /* "FB" */); put16(h, (uint32_t)(pad - 4)); h.insert(h.end(), pad - 4, 'Z'); }
        out(h.data(), h.size());
        out(r.data, r.size);
        put32(cd, 0x02014b50); put16(cd, 20); put16(cd, 20); put16(cd, 0); put16(cd, 0); put16(cd, 0); put16(cd, 0x21);
        put32(cd, crc); put32(cd, (uint32_t)r.size); put32(cd, (uint32_t)r.size);
        put16(cd, (uint32_t)nl); put16(cd, 0); put16(cd, 0); put16(cd, 0); put16(cd, 0); put32(cd, 0); put32(cd, lho);
        cd.insert(cd.end(), r.name.begin(), r.name.end());
    }
    if (off + cd.size() + 22 > LIMIT) throw Unsupported("archive larger than 4 GiB (zip64 is not written)");
    const uint32_t cdoff = (uint32_t)off;
    std::vector<uint8_t> e;
    put32(e, 0x06054b50); put16(e, 0); put16(e, 0); put16(e, (uint32_t)recs.size()); put16(e, (uint32_t)recs.size());
    put32(e, (uint32_t)cd.size()); put32(e, cdoff); put16(e, 0);
    out(cd.data(), cd.size());
    out(e.data(), e.size());
}

}  // namespace wdetail

// The kami network (nn.cpp:20-23,45-56) from a blob in the canonical order of include/kami_hip.h (`specs`: its
// blob_layout.h list for R residual blocks), written as the reference's module tree: attributes in its registration order,
// every BatchNorm with its int64 num_batches_tracked = bn_batches, then `generation`.  The file appears at `path` only
// once complete (temporary file in the same directory + rename).
// Throws Unsupported for a zip64-sized archive, std::runtime_error on an I/O failure.
inline void write_checkpoint(const std::string& path, int R, int64_t generation, int64_t bn_batches, const float* blob,
                             const std::vector<kh_blob::Tensor>& specs)
{
    using namespace wdetail;
    using T = kh_blob::Tensor;
    auto find = [&](const std::string& name) -> const T& {
        for (auto& t : specs) if (t.name == name) return t;
        throw std::logic_error("no tensor " + name);
    };

    // data.pkl, and the records its persistent ids name
    std::vector<Record> recs;
    const std::string root = "archive/";
    std::vector<std::string> keys;                             // (record names must outlive `recs`)
    const int nbn = 3 + 2 * R;
    std::vector<int64_t> counters((size_t)nbn, bn_batches);    // one int64 storage per BatchNorm, like libtorch's save
    keys.reserve(specs.size() + (size_t)nbn);
    Pickler pk;
    auto param = [&](const std::string& name, const char* leaf, bool is_param) {
        const T& t = find(name + "." + leaf);
        keys.push_back(std::to_string(keys.size()));
        pk.str(leaf);
        pk.tensor("FloatStorage", keys.back(), (int64_t)t.n, t.shape, is_param);
        recs.push_back({ root + "data/" + keys.back(), reinterpret_cast<const uint8_t*>(blob + t.at), t.n * 4 });
    };
    auto conv = [&](const std::string& attr, const std::string& name, const char* cls) {
        pk.str(attr); pk.begin_object(cls);
        param(name, "weight", true); param(name, "bias", true);
        pk.end_object();
    };
    int bn_seen = 0;
    auto bn = [&](const std::string& attr, const std::string& name) {
        pk.str(attr); pk.begin_object("BatchNorm2d");
        param(name, "weight", true); param(name, "bias", true);
        param(name, "running_mean", false); param(name, "running_var", false);
        keys.push_back(std::to_string(keys.size()));
        pk.str("num_batches_tracked");
        pk.tensor("LongStorage", keys.back(), 1, {}, false);
        recs.push_back({ root + "data/" + keys.back(), reinterpret_cast<const uint8_t*>(&counters[(size_t)bn_seen++]), 8 });
        pk.end_object();
    };
    pk.op(0x80); pk.b.push_back(2);                            // PROTO 2
    pk.begin_object("KamiNet");
    bn("batchnorm1", "batchnorm1");
    bn("vbatchnorm", "vbatchnorm");
    bn("pbatchnorm", "pbatchnorm");
    conv("conv1", "conv1", "Conv2d");
    conv("valueconv", "valueconv", "Conv2d");
    conv("policyconv", "policyconv", "Conv2d");
    conv("policyconv2", "policyconv2", "Conv2d");
    conv("valuefc", "valuefc", "Linear");
    for (int i = 0; i < R; ++i) {
        const std::string r = "residual" + std::to_string(i);
        pk.str(r); pk.begin_object("Residual");
        conv("conv1", r + ".conv1", "Conv2d");
        conv("conv2", r + ".conv2", "Conv2d");
        bn("batchnorm1", r + ".batchnorm1");
        bn("batchnorm2", r + ".batchnorm2");
        pk.end_object();
    }
    pk.str("generation"); pk.integer(generation);
    pk.end_object();
    pk.op(0x2e);                                               // STOP

    // the classes data.pkl names
    std::string code = "class KamiNet(Module):\n  __parameters__ = []\n  __buffers__ = []\n"
                       "  batchnorm1 : __torch__.BatchNorm2d\n  vbatchnorm : __torch__.BatchNorm2d\n  pbatchnorm : __torch__.BatchNorm2d\n"
                       "  conv1 : __torch__.Conv2d\n  valueconv : __torch__.Conv2d\n  policyconv : __torch__.Conv2d\n"
                       "  policyconv2 : __torch__.Conv2d\n  valuefc : __torch__.Linear\n";
    for (int i = 0; i < R; ++i) code += "  residual" + std::to_string(i) + " : __torch__.Residual\n";
    code += "  generation : int\n"
            "class Residual(Module):\n  __parameters__ = []\n  __buffers__ = []\n"
            "  conv1 : __torch__.Conv2d\n  conv2 : __torch__.Conv2d\n  batchnorm1 : __torch__.BatchNorm2d\n  batchnorm2 : __torch__.BatchNorm2d\n"
            "class BatchNorm2d(Module):\n  __parameters__ = [\"weight\", \"bias\", ]\n"
            "  __buffers__ = [\"running_mean\", \"running_var\", \"num_batches_tracked\", ]\n"
            "  weight : Tensor\n  bias : Tensor\n  running_mean : Tensor\n  running_var : Tensor\n  num_batches_tracked : Tensor\n"
            "class Conv2d(Module):\n  __parameters__ = [\"weight\", \"bias\", ]\n  __buffers__ = []\n  weight : Tensor\n  bias : Tensor\n"
            "class Linear(Module):\n  __parameters__ = [\"weight\", \"bias\", ]\n  __buffers__ = []\n  weight : Tensor\n  bias : Tensor\n";
    static const uint8_t constants[] = { 0x80, 0x02, 0x29, 0x2e };     // PROTO 2, EMPTY_TUPLE, STOP
    static const char version[] = "3\n", byteorder[] = "little";
    const std::string n_pkl = root + "data.pkl", n_code = root + "code/__torch__.py", n_const = root + "constants.pkl",
                      n_ver = root + "version", n_bo = root + "byteorder";
    recs.push_back({ n_pkl, pk.b.data(), pk.b.size() });
    recs.push_back({ n_code, reinterpret_cast<const uint8_t*>(code.data()), code.size() });
    recs.push_back({ n_const, constants, sizeof constants });
    recs.push_back({ n_ver, reinterpret_cast<const uint8_t*>(version), 2 });
    recs.push_back({ n_bo, reinterpret_cast<const uint8_t*>(byteorder), 6 });

    // atomic: a temporary file next to `path`, renamed over it once complete
    std::string tmpl = path + ".tmpXXXXXX";
    const int fd = mkstemp(&tmpl[0]);
    if (fd < 0) throw std::runtime_error("cannot create a file next to " + path + ": " + strerror(errno));
    (void)fchmod(fd, 0644);                                    // (mkstemp makes it 0600; a checkpoint is an ordinary file)
    FILE* f = fdopen(fd, "wb");
    if (!f) { const int err = errno; close(fd); unlink(tmpl.c_str()); throw std::runtime_error(std::string("fdopen: ") + strerror(err)); }
    try {
        write_zip(f, recs);
        if (fflush(f) != 0 || fsync(fileno(f)) != 0) throw std::runtime_error(std::string("write failed: ") + strerror(errno));
    } catch (...) {
        fclose(f);
        unlink(tmpl.c_str());
        throw;
    }
    if (fclose(f) != 0) { const int err = errno; unlink(tmpl.c_str()); throw std::runtime_error(std::string("write failed: ") + strerror(err)); }
    if (rename(tmpl.c_str(), path.c_str()) != 0) {
        const int err = errno;
        unlink(tmpl.c_str());
        throw std::runtime_error("cannot rename into " + path + ": " + strerror(err));
    }
}

}  // namespace kh_archive
