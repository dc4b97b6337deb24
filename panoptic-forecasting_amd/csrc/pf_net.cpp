#include "pf_net.h"

#include <cstring>

#include "pf_common.h"

namespace pf {

int parse_net_table(const void *blob, size_t bytes, int in_ch, int n_cls, NetTable &t) {
    if (bytes < sizeof(BlobHeader)) return fail(PF_EBLOB, "blob shorter than its header");
    BlobHeader &h = t.hdr;
    memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, kBlobMagic, 8) != 0 || h.version != kBlobVersion) return fail(PF_EBLOB, "bad blob magic/version");
    if (h.total_bytes != bytes || h.tensor_off + (uint64_t)h.n_tensors * sizeof(BlobTensor) > bytes ||
        h.op_off + (uint64_t)h.n_ops * sizeof(BlobOp) > bytes || h.weights_off > bytes || (h.weights_off & 3))
        return fail(PF_EBLOB, "blob table offsets out of range (total %llu, got %zu)", (unsigned long long)h.total_bytes, bytes);
    if ((int)h.in_ch != in_ch || (int)h.n_cls != n_cls)
        return fail(PF_EINVAL, "blob is for in_ch=%u n_cls=%u, caller asked for %d/%d", h.in_ch, h.n_cls, in_ch, n_cls);
    t.tensors.resize(h.n_tensors);
    t.ops.resize(h.n_ops);
    memcpy(t.tensors.data(), (const char *)blob + h.tensor_off, h.n_tensors * sizeof(BlobTensor));
    memcpy(t.ops.data(), (const char *)blob + h.op_off, h.n_ops * sizeof(BlobOp));
    for (size_t i = 0; i < t.ops.size(); ++i) {
        const BlobOp &o = t.ops[i];
        bool ok = o.n_src >= 1 && o.n_src <= (uint32_t)kConvMaxSrc && o.dst < h.n_tensors;
        for (uint32_t j = 0; ok && j < o.n_src; ++j)
            ok = o.src[j].tensor < h.n_tensors && o.src[j].choff + o.src[j].ch <= t.tensors[o.src[j].tensor].channels;
        if (!ok) return fail(PF_EBLOB, "op %zu is inconsistent with the tensor table", i);
    }
    return PF_OK;
}

int propagate_dims(const NetTable &t, int H, int W, std::vector<Dims> &d) {
    d.assign(t.tensors.size(), Dims());
    if (t.ops.empty()) return fail(PF_EBLOB, "empty op table");
    d[t.ops[0].src[0].tensor] = {H, W};
    for (const BlobOp &o : t.ops) {
        const Dims in = d[o.src[0].tensor];
        if (in.h <= 0 || in.w <= 0) return fail(PF_EBLOB, "op reads a tensor that was never produced");
        Dims out = in;
        switch (o.kind) {
            case OP_STEM:
            case OP_CONV: {
                const int pad = o.k / 2;
                out.h = (in.h + 2 * pad - (int)o.k) / (int)o.stride + 1;
                out.w = (in.w + 2 * pad - (int)o.k) / (int)o.stride + 1;
                break;
            }
            case OP_POOL: out = {in.h / 2, in.w / 2}; break;
            case OP_UPSAMPLE: out = d[o.src[1].tensor]; break;
            case OP_HEAD: break;
            default: return fail(PF_EBLOB, "unknown op kind %u", o.kind);
        }
        if (out.h <= 0 || out.w <= 0) return fail(PF_EINVAL, "input %dx%d is too small for this network", H, W);
        if (d[o.dst].h && (d[o.dst].h != out.h || d[o.dst].w != out.w) && o.kind != OP_HEAD)
            return fail(PF_EBLOB, "tensor %u written with two different sizes", o.dst);
        if (o.kind != OP_HEAD) d[o.dst] = out;
    }
    return PF_OK;
}

}  // namespace pf
