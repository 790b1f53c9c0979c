// rten_hip_graph.hpp -- ONNX loader + device-resident graph executor above rten_hip_ops.hpp (the
// "residency-aware executor glue" either side of the hot-path operators).
//
// What it mirrors in the reference, and where it stops:
//   * onnx::parse        rten-onnx/src/onnx.rs (hand-rolled protobuf reader, same subset: ModelProto / GraphProto /
//                        NodeProto / AttributeProto / TensorProto / ValueInfoProto), src/model/onnx_loader.rs
//                        (int64 initializers are narrowed to int32 at load, onnx_loader.rs:332-339).
//   * Graph::compile     Graph::prepack_weights (src/graph.rs:488-562: constant conv weights are staged once; prepacked_weight) and the
//                        fusion passes that touch this backend's operators (src/optimize/fusions.rs), each in one member:
//                        make_conv_step: Conv (+ Add residual) (+ Relu | activation); make_conv_integer_step: ConvInteger -> Cast -> Mul(scale)
//                        (= ConvIntegerToFloat, fusions.rs:1012-1058) (+ Add bias [1,O,1,1]) (+ Add residual) (+ Relu); make_matmul_integer_step:
//                        MatMulInteger -> Cast -> Mul (= MatMulIntegerToFloat); make_matmul_step: MatMul (+ scalar Mul / Div) (+ Add bias)
//                        (+ Gelu | Relu | activation) (= FusedMatMul); make_add_norm_step: Add -> LayerNormalization, Add -> Softmax;
//                        make_norm_step: InstanceNormalization | BatchNormalization (+ Relu | activation), LogSoftmax;
//                        plan_attention / emit_attention: the attention subgraph as MultiHeadSdpa; make_view_step: Reshape / Flatten / Squeeze /
//                        Unsqueeze / Identity as views.  compile() itself is the table of contents: it walks the nodes and dispatches to these.
//   * Graph::run         Graph::run_plan (src/graph.rs:1139-1231): operators run sequentially in plan order, values are
//                        reference counted and their buffers go back to the pool when the last consumer has run
//                        (buffer_pool.rs); here every value stays in HBM between operators -- only graph inputs and
//                        outputs cross PCIe.
// Scope of this first version: the CNN-classifier graphs of BASELINE configs 0-2 (ResNet-50 f32 and its
// dynamically-quantized form).  An operator outside the registry is a load-time error naming the node, never a CPU
// fallback.  Control flow, sequences, symbolic shape inference and the transformer-graph layout ops are not built.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <set>

#include "rten_hip_ops.hpp"

namespace rten_hip {

// ======================================================================================================== ONNX reader
namespace onnx {

enum DataType { FLOAT = 1, UINT8 = 2, INT8 = 3, INT32 = 6, INT64 = 7, BOOL = 9 };

struct TensorProto {
    std::string name;
    std::vector<int64_t> dims;
    int data_type = 0;
    std::string raw;                 // raw_data, or the typed fields re-encoded little-endian
    int64_t len() const { int64_t n = 1; for (int64_t d : dims) n *= d; return n; }
};
struct Attr {
    std::string name;
    int type = 0; // AttributeProto.AttributeType
    float f = 0.f;
    int64_t i = 0;
    std::string s;
    std::vector<float> floats;
    std::vector<int64_t> ints;
    std::vector<std::string> strings;
    TensorProto t;
};
struct Node {
    std::string op_type, name, domain;
    std::vector<std::string> inputs, outputs;
    std::vector<Attr> attrs;
    const Attr *attr(const std::string &n) const {
        for (auto &a : attrs) if (a.name == n) return &a;
        return nullptr;
    }
    int64_t get_int(const std::string &n, int64_t dflt) const { const Attr *a = attr(n); return a ? a->i : dflt; }
    float get_float(const std::string &n, float dflt) const { const Attr *a = attr(n); return a ? a->f : dflt; }
    std::vector<int> get_ints(const std::string &n, std::vector<int> dflt) const {
        const Attr *a = attr(n);
        if (!a) return dflt;
        return std::vector<int>(a->ints.begin(), a->ints.end());
    }
};
struct ValueInfo {
    std::string name;
    int elem_type = 0;
    std::vector<int64_t> dims; // -1: symbolic
    std::vector<std::string> dim_params;
};
struct Model {
    int64_t ir_version = 0, opset = 0;
    std::string producer, graph_name;
    std::vector<Node> nodes;
    std::vector<TensorProto> initializers;
    std::vector<ValueInfo> inputs, outputs;
    size_t folded_dequantize = 0; // canonical form only: DequantizeLinear nodes over initializers that became f32 initializers (Graph::canonicalize)
};

struct ParseError : std::runtime_error { using std::runtime_error::runtime_error; };

// protobuf wire format: (field << 3 | wire type) varint keys; wire 0 varint, 1 fixed64, 2 length-delimited, 5 fixed32
class Reader {
  public:
    Reader(const uint8_t *p, size_t n) : p_(p), end_(p + n) {}
    bool done() const { return p_ >= end_; }
    uint64_t varint() {
        uint64_t v = 0;
        for (int shift = 0; shift < 70; shift += 7) {
            if (p_ >= end_) throw ParseError("onnx: truncated varint");
            const uint8_t b = *p_++;
            v |= (uint64_t)(b & 0x7f) << shift;
            if (!(b & 0x80)) return v;
        }
        throw ParseError("onnx: varint too long");
    }
    void key(int &field, int &wire) { const uint64_t k = varint(); field = (int)(k >> 3); wire = (int)(k & 7); }
    Reader sub() {
        const uint64_t n = varint();
        if (n > (uint64_t)(end_ - p_)) throw ParseError("onnx: length-delimited field overruns its message");
        Reader r(p_, (size_t)n);
        p_ += n;
        return r;
    }
    std::string str() { Reader r = sub(); return std::string((const char *)r.p_, (size_t)(r.end_ - r.p_)); }
    uint32_t fixed32() { if (end_ - p_ < 4) throw ParseError("onnx: truncated fixed32"); uint32_t v; std::memcpy(&v, p_, 4); p_ += 4; return v; }
    uint64_t fixed64() { if (end_ - p_ < 8) throw ParseError("onnx: truncated fixed64"); uint64_t v; std::memcpy(&v, p_, 8); p_ += 8; return v; }
    void skip(int wire) {
        if (wire == 0) varint();
        else if (wire == 1) fixed64();
        else if (wire == 2) sub();
        else if (wire == 5) fixed32();
        else throw ParseError("onnx: unsupported wire type");
    }
    // repeated scalar: packed (wire 2) or one element (wire 0 / 5)
    template <typename F> void repeated(int wire, int scalar_wire, F f) {
        if (wire == 2) { Reader r = sub(); while (!r.done()) f(r); }
        else if (wire == scalar_wire) f(*this);
        else throw ParseError("onnx: unexpected wire type in a repeated scalar");
    }

  private:
    const uint8_t *p_, *end_;
};

inline TensorProto parse_tensor(Reader r) {
    TensorProto t;
    std::vector<float> fdata;
    std::vector<int64_t> i32data, i64data;
    bool has_raw = false;
    while (!r.done()) {
        int f, w;
        r.key(f, w);
        if (f == 1) r.repeated(w, 0, [&](Reader &q) { t.dims.push_back((int64_t)q.varint()); });
        else if (f == 2 && w == 0) t.data_type = (int)r.varint();
        else if (f == 4) r.repeated(w, 5, [&](Reader &q) { const uint32_t b = q.fixed32(); float v; std::memcpy(&v, &b, 4); fdata.push_back(v); });
        else if (f == 5) r.repeated(w, 0, [&](Reader &q) { i32data.push_back((int64_t)q.varint()); });
        else if (f == 7) r.repeated(w, 0, [&](Reader &q) { i64data.push_back((int64_t)q.varint()); });
        else if (f == 8 && w == 2) t.name = r.str();
        else if (f == 9 && w == 2) { t.raw = r.str(); has_raw = true; }
        else if (f == 13 || f == 14) throw ParseError("onnx: external tensor data is not supported (" + t.name + ")");
        else r.skip(w);
    }
    if (!has_raw) { // typed fields -> little-endian bytes of the declared type
        auto put = [&](const void *p, size_t n) { t.raw.append((const char *)p, n); };
        if (t.data_type == FLOAT) for (float v : fdata) put(&v, 4);
        else if (t.data_type == INT64) for (int64_t v : i64data) put(&v, 8);
        else if (t.data_type == INT32) for (int64_t v : i32data) { const int32_t x = (int32_t)v; put(&x, 4); }
        else if (t.data_type == UINT8 || t.data_type == INT8 || t.data_type == BOOL) for (int64_t v : i32data) { const uint8_t x = (uint8_t)v; put(&x, 1); }
    }
    return t;
}

inline Attr parse_attr(Reader r) {
    Attr a;
    while (!r.done()) {
        int f, w;
        r.key(f, w);
        if (f == 1 && w == 2) a.name = r.str();
        else if (f == 2 && w == 5) { const uint32_t b = r.fixed32(); std::memcpy(&a.f, &b, 4); }
        else if (f == 3 && w == 0) a.i = (int64_t)r.varint();
        else if (f == 4 && w == 2) a.s = r.str();
        else if (f == 5 && w == 2) a.t = parse_tensor(r.sub());
        else if (f == 7) r.repeated(w, 5, [&](Reader &q) { const uint32_t b = q.fixed32(); float v; std::memcpy(&v, &b, 4); a.floats.push_back(v); });
        else if (f == 8) r.repeated(w, 0, [&](Reader &q) { a.ints.push_back((int64_t)q.varint()); });
        else if (f == 9 && w == 2) a.strings.push_back(r.str());
        else if (f == 20 && w == 0) a.type = (int)r.varint();
        else r.skip(w);
    }
    return a;
}

inline Node parse_node(Reader r) {
    Node n;
    while (!r.done()) {
        int f, w;
        r.key(f, w);
        if (f == 1 && w == 2) n.inputs.push_back(r.str());
        else if (f == 2 && w == 2) n.outputs.push_back(r.str());
        else if (f == 3 && w == 2) n.name = r.str();
        else if (f == 4 && w == 2) n.op_type = r.str();
        else if (f == 5 && w == 2) n.attrs.push_back(parse_attr(r.sub()));
        else if (f == 7 && w == 2) n.domain = r.str();
        else r.skip(w);
    }
    return n;
}

inline ValueInfo parse_value_info(Reader r) {
    ValueInfo v;
    while (!r.done()) {
        int f, w;
        r.key(f, w);
        if (f == 1 && w == 2) v.name = r.str();
        else if (f == 2 && w == 2) { // TypeProto
            Reader tp = r.sub();
            while (!tp.done()) {
                int f2, w2;
                tp.key(f2, w2);
                if (f2 != 1 || w2 != 2) { tp.skip(w2); continue; } // tensor_type only
                Reader tt = tp.sub();
                while (!tt.done()) {
                    int f3, w3;
                    tt.key(f3, w3);
                    if (f3 == 1 && w3 == 0) v.elem_type = (int)tt.varint();
                    else if (f3 == 2 && w3 == 2) { // TensorShapeProto
                        Reader sh = tt.sub();
                        while (!sh.done()) {
                            int f4, w4;
                            sh.key(f4, w4);
                            if (f4 != 1 || w4 != 2) { sh.skip(w4); continue; }
                            Reader dm = sh.sub();
                            int64_t val = -1;
                            std::string param;
                            while (!dm.done()) {
                                int f5, w5;
                                dm.key(f5, w5);
                                if (f5 == 1 && w5 == 0) val = (int64_t)dm.varint();
                                else if (f5 == 2 && w5 == 2) param = dm.str();
                                else dm.skip(w5);
                            }
                            v.dims.push_back(val);
                            v.dim_params.push_back(param);
                        }
                    } else tt.skip(w3);
                }
            }
        } else r.skip(w);
    }
    return v;
}

inline Model parse(const uint8_t *data, size_t n) {
    Model m;
    Reader r(data, n);
    bool have_graph = false;
    while (!r.done()) {
        int f, w;
        r.key(f, w);
        if (f == 1 && w == 0) m.ir_version = (int64_t)r.varint();
        else if (f == 2 && w == 2) m.producer = r.str();
        else if (f == 8 && w == 2) { // OperatorSetIdProto
            Reader o = r.sub();
            std::string domain;
            int64_t version = 0;
            while (!o.done()) {
                int f2, w2;
                o.key(f2, w2);
                if (f2 == 1 && w2 == 2) domain = o.str();
                else if (f2 == 2 && w2 == 0) version = (int64_t)o.varint();
                else o.skip(w2);
            }
            if (domain.empty() || domain == "ai.onnx") m.opset = version;
        } else if (f == 7 && w == 2) {
            have_graph = true;
            Reader g = r.sub();
            while (!g.done()) {
                int f2, w2;
                g.key(f2, w2);
                if (f2 == 1 && w2 == 2) m.nodes.push_back(parse_node(g.sub()));
                else if (f2 == 2 && w2 == 2) m.graph_name = g.str();
                else if (f2 == 5 && w2 == 2) m.initializers.push_back(parse_tensor(g.sub()));
                else if (f2 == 11 && w2 == 2) m.inputs.push_back(parse_value_info(g.sub()));
                else if (f2 == 12 && w2 == 2) m.outputs.push_back(parse_value_info(g.sub()));
                else g.skip(w2);
            }
        } else r.skip(w);
    }
    if (!have_graph) throw ParseError("onnx: model has no graph");
    // graph inputs that are initializers are constants, not runtime inputs (IR < 4 models list both)
    std::set<std::string> init_names;
    for (auto &t : m.initializers) init_names.insert(t.name);
    m.inputs.erase(std::remove_if(m.inputs.begin(), m.inputs.end(), [&](const ValueInfo &v) { return init_names.count(v.name) != 0; }), m.inputs.end());
    return m;
}

inline Model load(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw ParseError("onnx: cannot open " + path);
    std::string buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    return parse((const uint8_t *)buf.data(), buf.size());
}

} // namespace onnx


// ======================================================================================================== shape arithmetic on the host
// Exporter-written graphs (PyTorch / transformers: dynamic-axis `view`s, position-id slices, attention-mask expansion) carry subgraphs whose VALUES depend only
// on input SHAPES and constants: Shape -> Gather -> Unsqueeze -> Concat -> Reshape, ConstantOfShape -> NonZero (an arange), index arithmetic, comparisons.
// The reference folds them at load against its symbolic shapes (`propagate_constants`, src/optimize.rs:705; shape inference in src/infer_shapes.rs).  This
// executor has no shape inference: it evaluates them ON THE HOST while a run walks the plan -- a step whose operands all carry a HostVal computes its result
// on the host and attaches it to a (cached) device copy; Reshape / Expand / Slice / ConstantOfShape read their shape operands from the HostVal.  A Graph
// may be run at other input shapes every time: each step caches the device copies of its latest 8 distinct values.  Within Graph::capture the shapes are
// fixed: the copies are made in its eager warm-up run and the captured hipGraph contains none of this arithmetic, only the copies' addresses -- which is why
// a copy a live capture may know is never released (Graph::materialize, Context::retire).  (The model ABI is stricter: it refuses bind_input after prepare.)
// Semantics follow the reference's operators (int32 everywhere: onnx_loader.rs:332-339; wrapping integer arithmetic; booleans 0 / 1).
namespace hostops {
constexpr int64_t kMaxHostElems = (int64_t)1 << 22; // beyond this a value is not worth mirroring on the host

inline int64_t wrap32(int64_t v) { return (int64_t)(int32_t)(uint32_t)(uint64_t)v; }
inline std::vector<int64_t> strides_for(const std::vector<int64_t> &shape, const std::vector<int64_t> &out) { // broadcast strides of `shape` on `out`
    std::vector<int64_t> st(out.size(), 0);
    int64_t acc = 1;
    for (size_t i = shape.size(); i-- > 0;) { st[out.size() - shape.size() + i] = shape[i] == 1 ? 0 : acc; acc *= shape[i]; }
    return st;
}
inline std::vector<int64_t> bshape(const std::vector<const HostVal *> &v) {
    std::vector<const std::vector<int64_t> *> sh;
    for (auto *x : v) sh.push_back(&x->shape);
    return broadcast_shapes(sh).shape;
}
// calls f(out_index, offsets[k]) for every element of the broadcast shape
template <typename F> void for_each_broadcast(const std::vector<int64_t> &out, const std::vector<std::vector<int64_t>> &st, F f) {
    int64_t n = 1;
    for (int64_t d : out) n *= d;
    std::vector<int64_t> idx(out.size(), 0), off(st.size(), 0);
    for (int64_t i = 0; i < n; i++) {
        f(i, off);
        for (size_t d = out.size(); d-- > 0;) {
            idx[d]++;
            for (size_t k = 0; k < st.size(); k++) off[k] += st[k][d];
            if (idx[d] < out[d]) break;
            for (size_t k = 0; k < st.size(); k++) off[k] -= st[k][d] * out[d];
            idx[d] = 0;
        }
    }
}
inline HostVal make_ints(std::vector<int64_t> shape, std::vector<int64_t> v) { HostVal h; h.shape = std::move(shape); h.i = std::move(v); return h; }

// Shape (src/ops/layout.rs:475-505): dims[start .. end) with negative bounds counted from the end and both clamped to [0, rank]
inline HostVal shape_of(const std::vector<int64_t> &dims, int64_t start, bool has_end, int64_t end) {
    const int64_t nd = (int64_t)dims.size();
    int64_t s = start < 0 ? start + nd : start, e = has_end ? (end < 0 ? end + nd : end) : nd;
    s = std::min(std::max<int64_t>(s, 0), nd); e = std::min(std::max<int64_t>(e, 0), nd);
    std::vector<int64_t> v;
    for (int64_t d = s; d < e; d++) v.push_back(dims[(size_t)d]);
    return make_ints({(int64_t)v.size()}, v);
}
inline bool logical_not(const HostVal &x, HostVal &out) { // unary_elementwise.rs:563-565
    if (x.is_float) return false;
    out.shape = x.shape;
    for (int64_t v : x.i) out.i.push_back(v == 0);
    return true;
}

// ---- element-wise: Add Sub Mul Div (both types), And Or Xor, Equal Less LessOrEqual Greater GreaterOrEqual
inline bool binary(const std::string &op, const HostVal &a, const HostVal &b, HostVal &out) {
    if (a.is_float != b.is_float) return false;
    out.shape = bshape({&a, &b});
    if (out.len() > kMaxHostElems) return false;
    const std::vector<std::vector<int64_t>> st{strides_for(a.shape, out.shape), strides_for(b.shape, out.shape)};
    const bool arith = op == "Add" || op == "Sub" || op == "Mul" || op == "Div";
    const bool logic = op == "And" || op == "Or" || op == "Xor";
    if (logic && a.is_float) return false;
    out.is_float = arith && a.is_float;
    const int64_t n = out.len();
    if (out.is_float) out.f.resize((size_t)n); else out.i.resize((size_t)n);
    bool ok = true;
    // Div (binary_elementwise.rs:613-637): an integer divisor that holds a zero anywhere is refused before anything is computed (check_nonzero); a float
    // divisor of exactly ONE element, at any rank, multiplies by its reciprocal -- a * (1 / b), two roundings -- and every other divisor divides
    if (op == "Div" && !a.is_float)
        for (int64_t y : b.i) if (y == 0) throw OpError(OpError::InvalidValue, "Divisor contains zero");
    const bool by_reciprocal = op == "Div" && a.is_float && b.len() == 1;
    const float reciprocal = by_reciprocal ? 1.f / b.f[0] : 0.f;
    for_each_broadcast(out.shape, st, [&](int64_t i, const std::vector<int64_t> &o) {
        if (a.is_float) {
            const float x = a.f[(size_t)o[0]], y = b.f[(size_t)o[1]];
            if (op == "Add") out.f[(size_t)i] = x + y; else if (op == "Sub") out.f[(size_t)i] = x - y; else if (op == "Mul") out.f[(size_t)i] = x * y;
            else if (op == "Div") out.f[(size_t)i] = by_reciprocal ? x * reciprocal : x / y;
            else if (op == "Equal") out.i[(size_t)i] = x == y; else if (op == "Less") out.i[(size_t)i] = x < y; else if (op == "LessOrEqual") out.i[(size_t)i] = x <= y;
            else if (op == "Greater") out.i[(size_t)i] = x > y; else if (op == "GreaterOrEqual") out.i[(size_t)i] = x >= y; else ok = false;
        } else {
            const int64_t x = a.i[(size_t)o[0]], y = b.i[(size_t)o[1]];
            int64_t r = 0;
            if (op == "Add") r = wrap32(x + y); else if (op == "Sub") r = wrap32(x - y); else if (op == "Mul") r = wrap32(x * y);
            else if (op == "Div") r = wrap32(x / y); // truncating; i32::MIN / -1 (a panic in the reference) wraps to i32::MIN, as on the device
            else if (op == "And") r = (x != 0) && (y != 0); else if (op == "Or") r = (x != 0) || (y != 0); else if (op == "Xor") r = (x != 0) != (y != 0);
            else if (op == "Equal") r = x == y; else if (op == "Less") r = x < y; else if (op == "LessOrEqual") r = x <= y;
            else if (op == "Greater") r = x > y; else if (op == "GreaterOrEqual") r = x >= y; else ok = false;
            out.i[(size_t)i] = r;
        }
    });
    return ok;
}
inline bool where(const HostVal &c, const HostVal &x, const HostVal &y, HostVal &out) {
    if (c.is_float || x.is_float != y.is_float) return false;
    out.shape = bshape({&c, &x, &y});
    if (out.len() > kMaxHostElems) return false;
    out.is_float = x.is_float;
    const std::vector<std::vector<int64_t>> st{strides_for(c.shape, out.shape), strides_for(x.shape, out.shape), strides_for(y.shape, out.shape)};
    if (out.is_float) out.f.resize((size_t)out.len()); else out.i.resize((size_t)out.len());
    for_each_broadcast(out.shape, st, [&](int64_t i, const std::vector<int64_t> &o) {
        const bool t = c.i[(size_t)o[0]] != 0;
        if (out.is_float) out.f[(size_t)i] = t ? x.f[(size_t)o[1]] : y.f[(size_t)o[2]];
        else out.i[(size_t)i] = t ? x.i[(size_t)o[1]] : y.i[(size_t)o[2]];
    });
    return true;
}
// Expand's shape checks (src/ops/layout.rs:106-118), shared by the host and the device path
inline void check_expand(const std::vector<int64_t> &shape, const std::vector<int64_t> &target) {
    for (int64_t d : target) if (d < 0) throw OpError(OpError::InvalidValue, "Target shape contains negative values");
    for (size_t i = 0; i < shape.size() && i < target.size(); i++) {
        const int64_t a = shape[shape.size() - 1 - i], b = target[target.size() - 1 - i];
        if (a != b && a != 1 && b != 1) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast input with target shape");
    }
}
inline HostVal expand(const HostVal &x, const std::vector<int64_t> &target) {
    check_expand(x.shape, target);
    HostVal out;
    out.is_float = x.is_float;
    HostVal t; t.shape = target;
    out.shape = bshape({&x, &t});
    const std::vector<std::vector<int64_t>> st{strides_for(x.shape, out.shape)};
    if (out.is_float) out.f.resize((size_t)out.len()); else out.i.resize((size_t)out.len());
    for_each_broadcast(out.shape, st, [&](int64_t i, const std::vector<int64_t> &o) { if (out.is_float) out.f[(size_t)i] = x.f[(size_t)o[0]]; else out.i[(size_t)i] = x.i[(size_t)o[0]]; });
    return out;
}
inline HostVal cast(const HostVal &x, DType to) { // src/ops/convert.rs: Rust `as`
    HostVal out;
    out.shape = x.shape;
    out.is_float = to == DType::F32;
    const size_t n = (size_t)x.len();
    if (out.is_float) { out.f.resize(n); for (size_t k = 0; k < n; k++) out.f[k] = x.is_float ? x.f[k] : (float)(int32_t)x.i[k]; return out; }
    out.i.resize(n);
    for (size_t k = 0; k < n; k++) {
        if (x.is_float) {
            const float f = x.f[k];
            const double lo = to == DType::I32 ? -2147483648.0 : to == DType::U8 ? 0.0 : -128.0, hi = to == DType::I32 ? 2147483647.0 : to == DType::U8 ? 255.0 : 127.0;
            out.i[k] = f != f ? 0 : (int64_t)std::trunc(std::min(std::max((double)f, lo), hi));
        } else {
            const int64_t v = x.i[k];
            out.i[k] = to == DType::I32 ? wrap32(v) : to == DType::U8 ? (v & 0xff) : (int64_t)(int8_t)(v & 0xff);
        }
    }
    return out;
}
inline HostVal reshaped(const HostVal &x, std::vector<int64_t> shape) { HostVal o = x; o.shape = std::move(shape); return o; }
inline HostVal transpose(const HostVal &x, const std::vector<int> &perm_in) {
    const int nd = (int)x.shape.size();
    std::vector<int> perm = perm_in;
    if (perm.empty()) for (int k = nd - 1; k >= 0; k--) perm.push_back(k);
    if ((int)perm.size() != nd) throw OpError(OpError::InvalidValue, "Permutation is invalid");
    std::vector<int64_t> xs((size_t)nd, 1);
    for (int d = nd - 2; d >= 0; d--) xs[(size_t)d] = xs[(size_t)d + 1] * x.shape[(size_t)d + 1];
    HostVal out;
    out.is_float = x.is_float;
    std::vector<int64_t> st((size_t)nd);
    unsigned seen = 0;
    for (int d = 0; d < nd; d++) {
        const int pd = perm[(size_t)d] < 0 ? perm[(size_t)d] + nd : perm[(size_t)d];
        if (pd < 0 || pd >= nd || (seen >> pd & 1u)) throw OpError(OpError::InvalidValue, "Permutation is invalid"); // (a repeated axis too: layout.rs:647-660)
        seen |= 1u << pd;
        out.shape.push_back(x.shape[(size_t)pd]);
        st[(size_t)d] = xs[(size_t)pd];
    }
    if (out.is_float) out.f.resize((size_t)out.len()); else out.i.resize((size_t)out.len());
    for_each_broadcast(out.shape, {st}, [&](int64_t i, const std::vector<int64_t> &o) { if (out.is_float) out.f[(size_t)i] = x.f[(size_t)o[0]]; else out.i[(size_t)i] = x.i[(size_t)o[0]]; });
    return out;
}
inline HostVal gather(const HostVal &x, const HostVal &ids, int axis) { // src/ops/gather.rs:21-110
    const int nd = (int)x.shape.size();
    if (nd < 1) throw OpError(OpError::InvalidValue, "Input must have >= 1 dims");
    const int ax = resolve_axis(axis, nd);
    const int64_t outer = detail::prod(x.shape, 0, (size_t)ax), alen = x.shape[(size_t)ax], inner = detail::prod(x.shape, (size_t)ax + 1, x.shape.size());
    HostVal out;
    out.is_float = x.is_float;
    out.shape.assign(x.shape.begin(), x.shape.begin() + ax);
    out.shape.insert(out.shape.end(), ids.shape.begin(), ids.shape.end());
    out.shape.insert(out.shape.end(), x.shape.begin() + ax + 1, x.shape.end());
    const int64_t nid = ids.len();
    for (int64_t o = 0; o < outer; o++)
        for (int64_t j = 0; j < nid; j++) {
            int64_t id = ids.i[(size_t)j];
            if (id < 0) id += alen;
            if (id < 0 || id >= alen) throw OpError(OpError::InvalidValue, "Entry in `indices` is out of range");
            for (int64_t k = 0; k < inner; k++) {
                const size_t src = (size_t)((o * alen + id) * inner + k);
                if (out.is_float) out.f.push_back(x.f[src]); else out.i.push_back(x.i[src]);
            }
        }
    return out;
}
// ---- CumSum / GatherElements / Trilu / Tile on host values: the arithmetic of the kernels in rten_amd/csrc/scan.hip (the f32 sum strictly sequential and
// starting as +0.0 + x0, int32 wrapping; the all-zero word where Trilu masks)
inline HostVal cumsum(const HostVal &x, int64_t axis, bool exclusive, bool reverse) { // reduce.rs:217-257
    if (axis < INT32_MIN || axis > INT32_MAX) throw OpError(OpError::InvalidValue, "Axis is invalid");
    const int ax = resolve_axis((int)axis, (int)x.shape.size());
    const int64_t outer = detail::prod(x.shape, 0, (size_t)ax), alen = x.shape[(size_t)ax], inner = detail::prod(x.shape, (size_t)ax + 1, x.shape.size());
    HostVal out;
    out.is_float = x.is_float;
    out.shape = x.shape;
    if (out.is_float) out.f.resize((size_t)out.len()); else out.i.resize((size_t)out.len());
    for (int64_t o = 0; o < outer; o++)
        for (int64_t k = 0; k < inner; k++) {
            volatile float facc = 0.f; // (volatile: every partial sum is stored as a float32, whatever the host compiler's excess precision)
            int64_t iacc = 0;
            for (int64_t t = 0; t < alen; t++) {
                const size_t at = (size_t)((o * alen + (reverse ? alen - 1 - t : t)) * inner + k);
                if (out.is_float) { const float prev = facc; facc = prev + x.f[at]; out.f[at] = exclusive ? prev : (float)facc; }
                else { const int64_t prev = iacc; iacc = wrap32(iacc + x.i[at]); out.i[at] = exclusive ? prev : iacc; }
            }
        }
    return out;
}
inline HostVal gather_elements(const HostVal &x, const HostVal &ids, int axis) { // gather.rs:196-284
    const int ax = check_gather_elements(x.shape, ids.shape, axis);
    const int nd = (int)x.shape.size();
    std::vector<int64_t> xs((size_t)nd, 1);
    for (int d = nd - 2; d >= 0; d--) xs[(size_t)d] = xs[(size_t)d + 1] * x.shape[(size_t)d + 1];
    HostVal out;
    out.is_float = x.is_float;
    out.shape = ids.shape;
    const int64_t n = out.len(), alen = x.shape[(size_t)ax];
    if (out.is_float) out.f.resize((size_t)n); else out.i.resize((size_t)n);
    std::vector<int64_t> idx((size_t)nd, 0);
    for (int64_t i = 0; i < n; i++) {
        int64_t id = ids.i[(size_t)i];
        if (id < 0) id += alen;
        if (id < 0 || id >= alen) throw OpError(OpError::InvalidValue, "Entry in `indices` is out of range");
        int64_t off = 0;
        for (int d = 0; d < nd; d++) off += (d == ax ? id : idx[(size_t)d]) * xs[(size_t)d];
        if (out.is_float) out.f[(size_t)i] = x.f[(size_t)off]; else out.i[(size_t)i] = x.i[(size_t)off];
        for (int d = nd - 1; d >= 0; d--) { if (++idx[(size_t)d] < out.shape[(size_t)d]) break; idx[(size_t)d] = 0; }
    }
    return out;
}
inline HostVal trilu(const HostVal &x, int64_t k, bool upper) { // trilu.rs:15-64, delta in 64 bits
    const size_t nd = x.shape.size();
    if (nd < 2) throw OpError(OpError::InvalidValue, "Input must have >= 2 dims");
    const int64_t rows = x.shape[nd - 2], cols = x.shape[nd - 1], n = x.len();
    const int64_t kc = std::max<int64_t>(-((int64_t)1 << 32), std::min<int64_t>((int64_t)1 << 32, k));
    HostVal out = x;
    for (int64_t i = 0; i < n; i++) {
        const int64_t col = i % cols, row = (i / cols) % rows, delta = row + kc - col;
        if (upper ? delta <= 0 : delta >= 0) continue;
        if (out.is_float) out.f[(size_t)i] = 0.f; else out.i[(size_t)i] = 0;
    }
    return out;
}
inline bool tile(const HostVal &x, const std::vector<int64_t> &repeats, HostVal &out) { // concat.rs:239-272; false: too large to mirror on the host
    out.is_float = x.is_float;
    out.shape = tiled_shape(x.shape, repeats);
    double total = 1;
    for (int64_t d : out.shape) total *= (double)d;
    if (total > (double)kMaxHostElems) return false;
    const size_t nd = x.shape.size();
    const int64_t n = out.len();
    std::vector<int64_t> xs(nd, 1);
    for (size_t d = nd; d-- > 1;) xs[d - 1] = xs[d] * x.shape[d];
    if (out.is_float) out.f.resize((size_t)n); else out.i.resize((size_t)n);
    std::vector<int64_t> idx(nd, 0);
    for (int64_t i = 0; i < n; i++) {
        int64_t off = 0;
        for (size_t d = 0; d < nd; d++) off += (idx[d] % x.shape[d]) * xs[d];
        if (out.is_float) out.f[(size_t)i] = x.f[(size_t)off]; else out.i[(size_t)i] = x.i[(size_t)off];
        for (size_t d = nd; d-- > 0;) { if (++idx[d] < out.shape[d]) break; idx[d] = 0; }
    }
    return true;
}
inline HostVal concat(const std::vector<const HostVal *> &v, int axis) { // src/ops/concat.rs
    const int nd = (int)v[0]->shape.size();
    const int ax = resolve_axis(axis, nd);
    HostVal out;
    out.is_float = v[0]->is_float;
    out.shape = v[0]->shape;
    out.shape[(size_t)ax] = 0;
    for (auto *x : v) {
        if ((int)x->shape.size() != nd) throw OpError(OpError::IncompatibleInputShapes, "Tensors must have the same number of dimensions");
        if (x->is_float != out.is_float) throw OpError(OpError::UnsupportedType, "");
        for (int d = 0; d < nd; d++)
            if (d != ax && x->shape[(size_t)d] != v[0]->shape[(size_t)d]) throw OpError(OpError::IncompatibleInputShapes, "Dimensions must be the same except for concat axis");
        out.shape[(size_t)ax] += x->shape[(size_t)ax];
    }
    const int64_t outer = detail::prod(out.shape, 0, (size_t)ax), inner = detail::prod(out.shape, (size_t)ax + 1, out.shape.size());
    for (int64_t o = 0; o < outer; o++)
        for (auto *x : v) {
            const int64_t row = x->shape[(size_t)ax] * inner;
            for (int64_t k = 0; k < row; k++) { if (out.is_float) out.f.push_back(x->f[(size_t)(o * row + k)]); else out.i.push_back(x->i[(size_t)(o * row + k)]); }
        }
    return out;
}
inline HostVal slice(const HostVal &x, const std::vector<SliceRange> &r) {
    const int nd = (int)x.shape.size();
    HostVal out;
    out.is_float = x.is_float;
    std::vector<int64_t> st((size_t)nd);
    int64_t acc = 1, base = 0;
    for (int d = nd - 1; d >= 0; d--) { out.shape.insert(out.shape.begin(), r[(size_t)d].count); st[(size_t)d] = acc * r[(size_t)d].step; base += acc * r[(size_t)d].start; acc *= x.shape[(size_t)d]; }
    if (out.is_float) out.f.resize((size_t)out.len()); else out.i.resize((size_t)out.len());
    for_each_broadcast(out.shape, {st}, [&](int64_t i, const std::vector<int64_t> &o) { if (out.is_float) out.f[(size_t)i] = x.f[(size_t)(base + o[0])]; else out.i[(size_t)i] = x.i[(size_t)(base + o[0])]; });
    return out;
}
inline HostVal nonzero(const HostVal &x) { // src/ops/reduce.rs:299-325: [rank, count] int32 indices of the non-zero elements, row-major order
    const int nd = (int)x.shape.size();
    std::vector<std::vector<int64_t>> cols;
    const int64_t n = x.len();
    std::vector<int64_t> idx((size_t)nd, 0);
    for (int64_t i = 0; i < n; i++) {
        const bool nz = x.is_float ? x.f[(size_t)i] != 0.f : x.i[(size_t)i] != 0;
        if (nz) cols.push_back(idx);
        for (int d = nd - 1; d >= 0; d--) { if (++idx[(size_t)d] < x.shape[(size_t)d]) break; idx[(size_t)d] = 0; }
    }
    HostVal out;
    out.shape = {(int64_t)nd, (int64_t)cols.size()}; // (a scalar input gives [0, 0 or 1]: reduce.rs:301-306)
    out.i.resize((size_t)(out.shape[0] * out.shape[1]));
    for (int d = 0; d < nd; d++) for (size_t c = 0; c < cols.size(); c++) out.i[(size_t)d * cols.size() + c] = cols[c][(size_t)d];
    return out;
}
// Range (src/ops/generate.rs:170-189): the reference's loop -- push `val`, then val = val + delta, while val is short of `limit` -- so that a float range
// has the reference's accumulated roundings and its element count.  Integers wrap at 32 bits.
inline HostVal range(const HostVal &start, const HostVal &limit, const HostVal &delta) {
    if (start.is_float != limit.is_float || start.is_float != delta.is_float) throw OpError(OpError::UnsupportedType, "");
    if (start.len() != 1) throw OpError(OpError::InvalidValue, "`start` must be a scalar");
    if (limit.len() != 1 || delta.len() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
    HostVal out;
    out.is_float = start.is_float;
    if (out.is_float) {
        const float l = limit.f[0], d = delta.f[0];
        if (d == 0.f) throw OpError(OpError::InvalidValue, "delta must be non-zero");
        for (float v = start.f[0]; (d > 0.f && v < l) || (d < 0.f && v > l); v = v + d) {
            if ((int64_t)out.f.size() >= kMaxHostElems) throw OpError(OpError::UnsupportedValue, "Range: too many elements");
            out.f.push_back(v);
        }
        out.shape = {(int64_t)out.f.size()};
    } else {
        const int64_t l = limit.i[0], d = delta.i[0];
        if (d == 0) throw OpError(OpError::InvalidValue, "delta must be non-zero");
        for (int64_t v = start.i[0]; d > 0 ? v < l : v > l; v = wrap32(v + d)) {
            if ((int64_t)out.i.size() >= kMaxHostElems) throw OpError(OpError::UnsupportedValue, "Range: too many elements");
            out.i.push_back(v);
        }
        out.shape = {(int64_t)out.i.size()};
    }
    return out;
}
// ConstantOfShape's one-element fill from the `value` attribute's int64 payload: saturated to int32 like every int64 initializer (onnx_loader.rs:464-492)
inline int64_t saturate32(int64_t v) { return std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v)); }
// ConstantOfShape (src/ops/generate.rs:18-29): `fill` (one element) over `shape`; a negative dimension is "Invalid shape"
inline HostVal constant_fill(const HostVal &fill, const std::vector<int64_t> &shape) {
    for (int64_t d : shape) if (d < 0) throw OpError(OpError::InvalidValue, "Invalid shape");
    return expand(fill, shape);
}
// The shape Flatten / Reshape / Squeeze / Unsqueeze give a tensor of `shape` (src/ops/layout.rs:231-240, 324-391, 560-600, 710-734), with the reference's
// checks in its order and words.  `spec`: Reshape's target or the axes; `axis`: Flatten's.
inline std::vector<int64_t> view_shape(const std::string &kind, const std::vector<int64_t> &shape, const std::vector<int64_t> &spec, bool have_spec, int axis, bool allowzero) {
    const int nd = (int)shape.size();
    const int64_t len = detail::prod(shape, 0, shape.size());
    if (kind == "Flatten") {
        const int a = axis < 0 ? axis + nd : axis;
        if (a < 0 || a > nd) throw OpError(OpError::InvalidValue, "Axis is invalid");
        return {detail::prod(shape, 0, (size_t)a), detail::prod(shape, (size_t)a, (size_t)nd)};
    }
    if (kind == "Reshape") {
        if (!have_spec) throw OpError(OpError::MissingInputs, "");
        std::vector<int64_t> s(spec);
        int64_t known = 1;
        int infer = -1;
        for (size_t i = 0; i < s.size(); i++) {
            if (s[i] < -1) throw OpError(OpError::InvalidValue, "Invalid dimension size in shape");
            if (s[i] == 0 && !allowzero) {
                if (i >= (size_t)nd) throw OpError(OpError::InvalidValue, "Zero dim has no corresponding input dim");
                s[i] = shape[i];
                known *= s[i];
            } else if (s[i] != -1) known *= s[i];
            else if (infer >= 0) throw OpError(OpError::InvalidValue, "Multiple dimensions in new shape set to -1");
            else infer = (int)i;
        }
        if (infer >= 0) {
            if (known == 0) throw OpError(OpError::InvalidValue, "Cannot infer size of -1 dim when other dims are zero");
            if (len % known != 0) throw OpError(OpError::InvalidValue, "Input length does not match target shape");
            s[(size_t)infer] = len / known;
        } else if (known != len) throw OpError(OpError::InvalidValue, "Input length does not match target shape");
        return s;
    }
    if (kind == "Squeeze") {
        std::vector<int64_t> o;
        std::vector<bool> drop((size_t)nd, false);
        for (int64_t a : spec) drop[(size_t)resolve_axis((int)a, nd)] = true;
        for (int i = 0; i < nd; i++) {
            if (have_spec ? drop[(size_t)i] : shape[(size_t)i] == 1) {
                if (shape[(size_t)i] != 1) throw OpError(OpError::InvalidValue, "Can only remove dimensions of size 1");
            } else o.push_back(shape[(size_t)i]);
        }
        return o;
    }
    if (kind == "Unsqueeze") {
        if (!have_spec) throw OpError(OpError::MissingInputs, "");
        const int out_nd = nd + (int)spec.size();
        std::vector<int64_t> o((size_t)out_nd, 0);
        std::vector<int> axes;
        for (int64_t a : spec) axes.push_back(resolve_axis((int)a, out_nd)); // ("Axis is invalid" before the uniqueness check)
        for (int a : axes) {
            if (o[(size_t)a] == 1) throw OpError(OpError::InvalidValue, "Axes must be unique");
            o[(size_t)a] = 1;
        }
        size_t src = 0;
        for (auto &d : o) if (d == 0) d = shape[src++];
        return o;
    }
    return shape; // Identity, Dropout
}
// The walk the host reductions over sorted unique `axes` share (src/ops/reduce.rs:414-520): gives `y` its shape, calls init(n) with the number of output
// elements, then fold(o, e) for every element e of `x` in row-major order, o being the output element whose slice holds it
template <class Init, class Fold>
inline void reduce_walk(const HostVal &x, const std::vector<int> &axes, bool keep_dims, HostVal &y, Init init, Fold fold) {
    const size_t nd = x.shape.size();
    std::vector<int64_t> kept_stride(nd, 0), idx(nd, 0);
    auto reduced = [&](size_t d) { return std::find(axes.begin(), axes.end(), (int)d) != axes.end(); };
    int64_t acc = 1;
    for (size_t d = nd; d-- > 0;)
        if (!reduced(d)) { kept_stride[d] = acc; acc *= x.shape[d]; }
    for (size_t d = 0; d < nd; d++) {
        if (!reduced(d)) y.shape.push_back(x.shape[d]);
        else if (keep_dims) y.shape.push_back(1);
    }
    init((size_t)acc);
    for (int64_t e = 0, n = x.len(); e < n; e++) {
        int64_t o = 0;
        for (size_t d = 0; d < nd; d++) o += idx[d] * kept_stride[d];
        fold((size_t)o, (size_t)e);
        for (size_t d = nd; d-- > 0;) { if (++idx[d] < x.shape[d]) break; idx[d] = 0; }
    }
}
// ReduceMax / ReduceMin of a host value (shape arithmetic sometimes takes the extreme of a shape vector): NaN propagates, an empty slice gives the identity
// (src/ops/reduce.rs:876-1044)
inline HostVal reduce_minmax(const HostVal &x, const std::vector<int> &axes, bool keep_dims, bool min) {
    HostVal y;
    y.is_float = x.is_float;
    const float fid = min ? std::numeric_limits<float>::infinity() : -std::numeric_limits<float>::infinity();
    const int64_t iid = min ? std::numeric_limits<int32_t>::max() : std::numeric_limits<int32_t>::min();
    reduce_walk(x, axes, keep_dims, y, [&](size_t n) { if (x.is_float) y.f.assign(n, fid); else y.i.assign(n, iid); }, [&](size_t o, size_t e) {
        if (x.is_float) {
            float &a = y.f[o];
            const float b = x.f[e];
            if (a != a) {} else if (b != b) a = std::numeric_limits<float>::quiet_NaN(); else a = min ? std::min(a, b) : std::max(a, b);
        } else {
            int64_t &a = y.i[o];
            a = min ? std::min(a, x.i[e]) : std::max(a, x.i[e]);
        }
    });
    return y;
}
// int32 ReduceL1 / ReduceSumSquare / ReduceProd of a host value (dynamic-axes exports take ReduceProd of a Shape): two's complement wrapping arithmetic,
// as the device kernels and the reference's generic kernels in a release build (src/ops/reduce.rs:782-794,1052-1057,1174-1181); an empty slice gives 0
// (Prod: 1).  `kind`: RTEN_HIP_REDUCE_L1 / _SUM_SQUARE / _PROD.
inline HostVal reduce_i32(const HostVal &x, const std::vector<int> &axes, bool keep_dims, int kind) {
    HostVal y;
    y.is_float = false;
    std::vector<uint32_t> r;
    reduce_walk(x, axes, keep_dims, y, [&](size_t n) { r.assign(n, kind == RTEN_HIP_REDUCE_PROD ? 1u : 0u); }, [&](size_t o, size_t e) {
        const uint32_t v = (uint32_t)(int32_t)x.i[e];
        if (kind == RTEN_HIP_REDUCE_L1) r[o] += (v & 0x80000000u) ? 0u - v : v;
        else if (kind == RTEN_HIP_REDUCE_SUM_SQUARE) r[o] += v * v;
        else r[o] *= v;
    });
    for (uint32_t v : r) y.i.push_back((int64_t)(int32_t)v);
    return y;
}
// ---- unary math of a host value, with the device's semantics (all exact in C++): Neg / Abs / Sign for both types (int32 wraps: i32::MIN stays; float Sign is
// Rust's signum: +0 -> 1, -0 -> -1, NaN -> NaN), Floor / Ceil / Round (ties to even) / Sqrt / Reciprocal for float32.  false: not this operator / type.
inline bool unary(const std::string &op, const HostVal &x, HostVal &out) {
    out = HostVal();
    out.shape = x.shape;
    out.is_float = x.is_float;
    if (!x.is_float) {
        if (op != "Neg" && op != "Abs" && op != "Sign") return false;
        for (int64_t v : x.i) out.i.push_back(op == "Neg" ? wrap32(-v) : op == "Abs" ? wrap32(v < 0 ? -v : v) : (int64_t)(v > 0) - (int64_t)(v < 0));
        return true;
    }
    for (float v : x.f) {
        float r;
        uint32_t w;
        std::memcpy(&w, &v, 4);
        if (op == "Neg") { w ^= 0x80000000u; std::memcpy(&r, &w, 4); }
        else if (op == "Abs") { w &= 0x7fffffffu; std::memcpy(&r, &w, 4); }
        else if (op == "Sign") r = v != v ? std::numeric_limits<float>::quiet_NaN() : std::copysign(1.0f, v);
        else if (op == "Floor") r = std::floor(v);
        else if (op == "Ceil") r = std::ceil(v);
        else if (op == "Round") r = std::nearbyint(v); // the default rounding mode: ties to even
        else if (op == "Sqrt") r = std::sqrt(v);
        else if (op == "Reciprocal") r = 1.0f / v;
        else return false;
        out.f.push_back(r);
    }
    return true;
}
// Min / Max of two host values (reduce.rs:847-873: a NaN in either operand wins, a tie keeps `a`), numpy broadcasting
inline bool minmax(bool is_min, const HostVal &a, const HostVal &b, HostVal &out) {
    if (a.is_float != b.is_float) return false;
    out = HostVal();
    out.shape = bshape({&a, &b});
    if (out.len() > kMaxHostElems) return false;
    out.is_float = a.is_float;
    const std::vector<std::vector<int64_t>> st{strides_for(a.shape, out.shape), strides_for(b.shape, out.shape)};
    if (out.is_float) out.f.resize((size_t)out.len()); else out.i.resize((size_t)out.len());
    for_each_broadcast(out.shape, st, [&](int64_t i, const std::vector<int64_t> &o) {
        if (out.is_float) {
            const float x = a.f[(size_t)o[0]], y = b.f[(size_t)o[1]];
            out.f[(size_t)i] = x != x ? x : (y != y ? y : ((is_min ? x <= y : x >= y) ? x : y));
        } else {
            const int64_t x = a.i[(size_t)o[0]], y = b.i[(size_t)o[1]];
            out.i[(size_t)i] = (is_min ? x <= y : x >= y) ? x : y;
        }
    });
    return true;
}
// variadic Min / Max: one operand is a copy, otherwise a left fold
inline bool minmax_fold(bool is_min, const std::vector<const HostVal *> &v, HostVal &out) {
    if (v.empty() || !v[0]) return false;
    HostVal acc = *v[0];
    for (size_t k = 1; k < v.size(); k++) {
        if (!v[k]) return false;
        HostVal next;
        if (!minmax(is_min, acc, *v[k], next)) return false;
        acc = std::move(next);
    }
    out = std::move(acc);
    return true;
}
// Pad of a host value in constant mode (src/ops/pad.rs:34-108; exporters pad shape vectors): negative entries crop first
inline bool pad_constant(const HostVal &x, const std::vector<int64_t> &pads, const HostVal *value, HostVal &out) {
    if (value && (value->is_float != x.is_float || !value->shape.empty())) return false;
    const PadGeometry g = pad_geometry(x.shape, pads, RTEN_HIP_PAD_CONSTANT);
    const size_t nd = x.shape.size();
    out = HostVal();
    out.shape = g.out;
    out.is_float = x.is_float;
    if (out.len() > kMaxHostElems) return false;
    const float ff = value && x.is_float ? value->f.at(0) : 0.f;
    const int64_t fi = value && !x.is_float ? value->i.at(0) : 0;
    if (out.is_float) out.f.assign((size_t)out.len(), ff); else out.i.assign((size_t)out.len(), fi);
    std::vector<int64_t> xs(nd, 1), idx(nd, 0);
    for (size_t d = nd; d-- > 1;) xs[d - 1] = xs[d] * x.shape[d];
    for (int64_t e = 0, n = out.len(); e < n; e++) {
        int64_t src = 0;
        bool inside = true;
        for (size_t d = 0; d < nd; d++) {
            const int64_t s = idx[d] - pads[d]; // (a negative begin pad shifts into the cropped region)
            const int64_t hi = x.shape[d] - std::max<int64_t>(-pads[nd + d], 0), lo = std::max<int64_t>(-pads[d], 0);
            inside = inside && s >= lo && s < hi;
            src += s * xs[d];
        }
        if (inside) { if (out.is_float) out.f[(size_t)e] = x.f[(size_t)src]; else out.i[(size_t)e] = x.i[(size_t)src]; }
        for (size_t d = nd; d-- > 0;) { if (++idx[d] < out.shape[d]) break; idx[d] = 0; }
    }
    return true;
}
} // namespace hostops

// ======================================================================================================== executor
struct GraphError : std::runtime_error { using std::runtime_error::runtime_error; };

class Graph {
  public:
    struct Options {
        bool fuse = true;    // the fusion passes listed at the top of this file
        bool prepack = true; // stage constant conv weights once (Graph::prepack_weights)
        // Opt-in, per edge (a launch plan: profiles/plans/int8.json "qout"): ConvInteger nodes, by name, whose fused ConvIntegerToFloat step also
        // runs the DynamicQuantizeLinear of the one convolution reading its output (rten_hip_conv2d_int8_qout).  That launch needs the device to
        // itself (all its workgroups resident at once; rten_hip.h states the time-out contract), so it is never a default.
        std::set<std::string> qout;
        // The same edges in the RECOMPUTE form (plan key "qout2"; round 6): the producing convolution runs twice -- statistics only, then again with the
        // consumer's codes as its output -- so there is no grid-wide exchange and no residency requirement: replicas side by side ("lanes") may use it.  The
        // f32 tensor of the edge is never written or read back (8 B per element of HBM traffic saved for one more pass over small int8 operands).
        std::set<std::string> qout_recompute;
        // Opt-in, per layer (profiles/plans/int8.json "fused_dql"): pointwise ConvInteger nodes, by name, whose fused ConvIntegerToFloat step runs its
        // DynamicQuantizeLinear inside its own operand loader (rten_hip_conv2d_int8_dql) instead of reading the staged codes.
        std::set<std::string> fused_dql;
        // Opt-in, per layer (a launch plan: profiles/plans/f32_lanes.json "pairs"): f32 Conv steps, by name, that also run the ONE pointwise convolution reading
        // their output -- a bottleneck block's expand layer and the next block's reduce layer in one launch (rten_hip_conv2d_f32_pair; round 6): the
        // second layer takes its operand from LDS instead of reading the tensor back from HBM.  Same bits; a pair the kernel has no form for runs as two launches.
        std::set<std::string> pairs;
        // ... and, of those, the pairs that ALSO compute their first convolution's residual in the launch (plan key "pair_shortcuts"): the residual is the output of a
        // 64-channel pointwise Conv step nothing else reads -- a stage's shortcut layer -- which then has no launch and no tensor of its own
        // (rten_hip_conv2d_f32_pair_shortcut).
        std::set<std::string> pair_shortcuts;
        // A rank that RECEIVES the weight arena (coalesce_constants() + one broadcast from the rank that loaded the file for real): initializers of
        // 64 KB and more are allocated but not uploaded.  Everything derived from them on the device (prepacked weights) is computed on whatever the
        // buffers hold and overwritten by the broadcast, which covers every constant buffer of the graph.
        bool skip_large_uploads = false;
    };
    struct Timing { std::string node, op; double ms; };

    Graph(Context &ctx, const onnx::Model &m, Options opt) : ctx_(ctx), opt_(opt) { compile(m); }
    Graph(Context &ctx, const onnx::Model &m) : Graph(ctx, m, Options()) {}
    // A second plan over the SAME model that shares `donor`'s device constants and prepacked weights instead of uploading its own (the sub-batch
    // chains of one model: four copies of a 100 MB weight set would also compete for the same L2 / MALL lines).  `donor` must outlive this graph
    // and live on the same device; both must have been built with the same options.
    Graph(Context &ctx, const onnx::Model &m, Options opt, const Graph &donor) : ctx_(ctx), opt_(opt), donor_(&donor) { compile(m); }
    // the node list after the load-time canonicalisation of exporter idioms (Constant nodes, GeluFusion, LayerNormalizationFusion): needs no device
    static onnx::Model canonical_form(const onnx::Model &m) { return canonicalize(m); }

    const std::vector<onnx::ValueInfo> &inputs() const { return inputs_; }
    const std::vector<onnx::ValueInfo> &outputs() const { return outputs_; }
    size_t num_steps() const { return steps_.size(); }
    size_t num_fused_away() const { return fused_away_; }
    size_t num_staged_quantizers() const { return staged_dql_; }
    size_t num_qout_edges() const { return qout_edges_; } // quantizers merged into their producer's launch (Options::qout)
    size_t num_stats_blocks() const { return stats_blocks_; }
    size_t num_conv_pairs() const { return conv_pairs_; } // convolution pairs that run as one launch (Options::pairs)
    size_t num_dql_loader_steps() const { return dql_loader_steps_; } // convolutions that quantize in their own loader (Options::fused_dql)

    // Moves every device constant of this graph -- uploaded initializers, constants derived at load (merged QKV weights), prepacked conv / MatMul
    // weights -- into ONE allocation, in a deterministic order (value id, then prepack order): the weight arena a batch-sharded deployment
    // broadcasts once from the rank that read the model file (RCCL over xGMI).  Two processes that load the same model with the same
    // options get the same layout.  Must run before a sharing graph (the `donor` constructor) is built on this one and before any capture.
    std::pair<void *, size_t> coalesce_constants() {
        if (donor_) throw GraphError("coalesce_constants: a graph that shares a donor's constants has none of its own");
        if (arena_) return {arena_->ptr(), (size_t)arena_->len()};
        auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
        size_t total = 0;
        for (auto &kv : consts_) total += pad(kv.second.bytes());
        for (auto &pk : packed_) total += pad(pk->bytes());
        arena_.reset(new Tensor(ctx_, {(int64_t)std::max<size_t>(total, 256)}, DType::U8));
        size_t off = 0;
        auto move_in = [&](Tensor &t) {
            const size_t b = t.bytes();
            if (b) ctx_.check(rten_hip_memcpy_d2d(ctx_.raw(), (char *)arena_->ptr() + off, t.ptr(), b));
            Tensor v = Tensor::view_at(*arena_, off, t.shape(), t.dtype());
            v.set_host(t.host_ptr()); // a small constant's host mirror (shape arithmetic reads it) moves with it
            ctx_.sync();       // the copy has read the old buffer before it goes back to the allocator
            t = std::move(v);  // same Tensor object (steps hold pointers to it), new storage
            off += pad(b);
        };
        for (auto &kv : consts_) move_in(kv.second);
        for (auto &pk : packed_) move_in(*pk);
        ctx_.trim_pool();
        return {arena_->ptr(), (size_t)arena_->len()};
    }

    // Empty, or the first step whose result for one row of dim 0 depends on the other rows: such a graph cannot be split into sub-batch chains
    // (DynamicQuantizeLinear takes its min / max over the whole tensor; a reduction / normalisation over axis 0 mixes rows).
    std::string batch_coupled_step() const {
        for (auto &st : steps_) if (st.batch_coupled) return st.kind_name + " \"" + st.name + "\"";
        return "";
    }
    // ... and what only a RUN can tell (ranks are run-time facts here): a Softmax / LayerNormalization / ReduceSum / ReduceMean whose NEGATIVE axis resolved to
    // dim 0, or a device Transpose that moved dim 0.  Empty, or the first such step of the last run (rten_hip_model_prepare checks it after its probe run).
    const std::string &runtime_batch_coupled_step() const { return runtime_coupled_; }
    // Empty, or the first step that reads a value back from the device to shape its output (NonMaxSuppression's row count): a plan that holds one runs
    // eagerly, clones and lanes included, and cannot be captured.  Known from the plan, without a run.
    std::string reading_back_step() const {
        for (auto &st : steps_) if (st.reads_back) return st.kind_name + " \"" + st.name + "\"";
        return "";
    }
    static std::string capture_refusal(const std::string &step) {
        return step + " reads its row count back from the device: a graph whose output shape depends on device values cannot be captured (run it eagerly)";
    }
    std::vector<std::string> step_names() const {
        std::vector<std::string> v;
        for (auto &s : steps_) v.push_back(s.kind_name + ":" + s.name);
        return v;
    }

    // Runs the plan.  `feeds` are device tensors named like the graph inputs; the returned tensors are the graph outputs
    // in declaration order, still on the device.  With `timings`, every step is followed by a sync and timed on the host
    // (RTEN_TIMING's per-operator table, src/timing.rs) -- a profiling aid, it serialises the stream.
    using Feeds = std::vector<std::pair<std::string, const Tensor *>>;

    // Load-time plan selection: one pass over the graph in which every f32 convolution step times its candidate launch
    // plans on its real operands (tile variant x exact split-K plan x tile order, the candidate set of
    // rten_amd/workloads/resnet50.py::candidate_plans) and keeps the fastest.  Returns the number of tuned steps.
    size_t autotune(const Feeds &feeds, int reps = 3) {
        tune_reps_ = reps;
        tuned_ = 0;
        run(feeds);
        ctx_.sync();
        tune_reps_ = 0;
        return tuned_;
    }

    // A committed launch plan instead of timing at load ({conv step name: GemmPlan}, profiles/plans/*.json: tuned once on an MI355X so that
    // every process -- and every rank of a sharded deployment -- launches the same kernels).  Steps the table does not name keep the
    // backend's automatic plan.  Returns the number of steps that took an entry.
    size_t apply_plan(const std::map<std::string, GemmPlan> &table) {
        size_t n = 0;
        for (auto &st : steps_) {
            if (!st.conv && !st.gemm_plan && !st.i8) continue;
            auto it = table.find(st.name);
            if (it == table.end()) { if (st.i8) st.i8->tile = -1; continue; }
            if (st.i8) { // an int8 convolution step: the entry's first number is its workgroup tile (round 6: "<step>": [tile, 0, 1, 0])
                if (it->second.variant < 0 || it->second.variant > 3) continue;
                st.i8->tile = it->second.variant;
            }
            else if (st.conv) st.conv->plan = it->second;
            else *st.gemm_plan = it->second;
            n++;
        }
        return n;
    }
    // Plan entries keyed by the PRODUCT'S SHAPE -- "gemm:MxKxN", M = the rows of A over all its leading dims -- for MatMul-family steps no name entry covers (round
    // 6): a plan chosen on one writer's graph (profiles/plans/bert_base_b32_s128_lanes.json, its "shapes" table) then applies to another exporter's file of
    // the same model, whose steps carry other names.  Shapes are run-time facts here, so the lookup happens in run(), once per step (the entry stays).
    void set_shape_plans(std::map<std::string, GemmPlan> t) {
        for (size_t i : shape_planned_steps_) *steps_[i].gemm_plan = GemmPlan{}; // (a re-plan: entries a previous table left on steps go with that table)
        shape_planned_steps_.clear();
        shape_plans_ = std::move(t);
        shape_planned_ = 0;
    }
    size_t num_shape_planned() const { return shape_planned_; }
    std::map<std::string, GemmPlan> plans() const { // what autotune() / apply_plan() left on the convolution steps
        std::map<std::string, GemmPlan> t;
        for (auto &st : steps_) {
            if (st.conv && st.conv->plan.set) t[st.name] = st.conv->plan;
            if (st.gemm_plan && st.gemm_plan->set) t[st.name] = *st.gemm_plan;
            if (st.i8 && st.i8->tile >= 0) t[st.name] = GemmPlan{true, st.i8->tile, 0, 1, 0};
        }
        return t;
    }
    bool captured() const { return graph_ != 0; }
    const std::vector<Tensor> &captured_outputs() const { return captured_outputs_; }

    // hipGraph capture of one run (launch-bound at small batch: ~60 operators of 5-50 us).  The feeds and the returned
    // outputs keep their device addresses: write new inputs into the same feed tensors, call replay(), read the outputs.
    // The captured graph's intermediates live in the context's buffer pool: every replay rewrites them, so between replays the pool may serve others --
    // eager runs of this Graph at other shapes included -- but it must not be trimmed, and nothing may use it WHILE a replay is in flight on another stream.
    // What the captured graph only reads -- the steps' cached shape constants and reciprocals -- stays in place for as long as the capture lives.
    // `tail` (optional) runs at the end of the captured region, on the capturing stream, with the run's outputs: work recorded there -- e.g. the
    // copy of a sub-batch's rows into a resident full-batch tensor -- replays with the graph.
    // A plan with a step that reads back (reading_back_step) is refused here, from the plan, before the warm-up run and before any stream capture begins: the
    // refusal is never discovered by synchronising inside an active capture, and a graph captured earlier stays as it is.
    const std::vector<Tensor> &capture(const Feeds &feeds, const std::function<void(const std::vector<Tensor> &)> &tail = nullptr) {
        { const std::string rb = reading_back_step(); if (!rb.empty()) throw GraphError("capture: " + capture_refusal(rb)); }
        run(feeds); // warm: every buffer size is in the pool, scratch is grown, code objects are loaded
        ctx_.sync();
        if (graph_) { // re-capture: the previous executable graph is released first
            ctx_.check(rten_hip_graph_destroy(ctx_.raw(), graph_));
            graph_ = 0;
            ctx_.capture_destroyed();
        }
        ctx_.check(rten_hip_graph_begin(ctx_.raw()));
        try {
            captured_outputs_ = run(feeds);
            if (tail) tail(captured_outputs_);
        } catch (...) { // leave the stream (and the context's lock) out of capture mode before the error propagates
            uint64_t dead = 0;
            if (rten_hip_graph_end(ctx_.raw(), &dead) == RTEN_HIP_OK && dead) rten_hip_graph_destroy(ctx_.raw(), dead);
            throw;
        }
        ctx_.check(rten_hip_graph_end(ctx_.raw(), &graph_));
        if (graph_) ctx_.capture_made(); // from here on the steps' cached device copies stay where they are (Context::retire)
        return captured_outputs_;
    }
    void replay() {
        if (!graph_) throw GraphError("replay: no captured graph");
        ctx_.check(rten_hip_graph_launch(ctx_.raw(), graph_));
    }
    ~Graph() { if (graph_) { rten_hip_graph_destroy(ctx_.raw(), graph_); ctx_.capture_destroyed(); } }
    Graph(const Graph &) = delete;
    Graph &operator=(const Graph &) = delete;

    std::vector<Tensor> run(const Feeds &feeds, std::vector<Timing> *timings = nullptr) {
        std::vector<const Tensor *> val(names_.size(), nullptr);
        std::vector<std::unique_ptr<Tensor>> owned(names_.size());
        std::vector<int> pending(uses_);
        runtime_coupled_.clear();
        for (auto &kv : consts_) val[(size_t)kv.first] = &kv.second;
        for (auto &fd : feeds) {
            auto it = ids_.find(fd.first);
            if (it == ids_.end()) throw GraphError("run: no graph input named " + fd.first);
            val[(size_t)it->second] = fd.second;
        }
        for (auto &in : inputs_) if (!val[(size_t)ids_.at(in.name)]) throw GraphError("run: missing input " + in.name);
        if (stats_blocks_) ctx_.check(rten_hip_minmax_stats_reset(ctx_.raw(), stats_arena_->ptr(), (int32_t)stats_blocks_)); // one launch for every block
        for (auto &st : steps_) {
            InputList in;
            for (int id : st.in) {
                if (id >= 0 && !val[(size_t)id]) throw GraphError("run: value " + names_[(size_t)id] + " needed by " + st.name + " was never produced");
                in.push_back(id < 0 ? nullptr : val[(size_t)id]);
            }
            const auto t0 = std::chrono::steady_clock::now();
            OutputList out;
            if (st.gemm_plan && !st.gemm_plan->set && !shape_plans_.empty() && tune_reps_ == 0 && in.size() > 1 && in[0] && in[1] && in[0]->ndim() >= 2 && in[1]->ndim() == 2) {
                const Tensor &a = *in[0], &b = *in[1];
                const int64_t k = a.size(a.ndim() - 1), mrows = a.len() / std::max<int64_t>(k, 1);
                const int64_t ncols = b.size(0) == k ? b.size(1) : (b.size(1) == k ? b.size(0) : -1); // [K, N], or [N, K] (Gemm with transB)
                auto it = ncols < 0 ? shape_plans_.end() : shape_plans_.find("gemm:" + std::to_string(mrows) + "x" + std::to_string(k) + "x" + std::to_string(ncols));
                if (it != shape_plans_.end()) { *st.gemm_plan = it->second; shape_planned_++; shape_planned_steps_.push_back((size_t)(&st - steps_.data())); }
            }
            if (tune_reps_ > 0 && (st.conv || st.gemm_plan)) tune_step(st, in);
            try {
                if (st.i8 && st.i8->tile >= 0) { // the plan's workgroup tile around this step's launches (the caller's own setting comes back)
                    struct TileScope {
                        Context &c; int32_t prev = -1; bool on = false;
                        TileScope(Context &c_, int tile) : c(c_) { on = rten_hip_set_int8_tile(c.raw(), tile, &prev) == RTEN_HIP_OK; }
                        ~TileScope() { if (on) rten_hip_set_int8_tile(c.raw(), prev, nullptr); }
                    } scope(ctx_, st.i8->tile);
                    out = st.run(ctx_, in);
                } else
                out = st.run(ctx_, in);
            } catch (const OpError &e) { // name the node, like the reference's RunError::OperatorError { name, error }
                throw OpError(e.kind, "operator " + st.kind_name + " \"" + st.name + "\": " + e.msg);
            }
            if (timings) {
                ctx_.sync();
                timings->push_back({st.name, st.kind_name, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()});
            }
            if (out.size() < st.out.size()) throw GraphError("run: " + st.name + " produced fewer outputs than the graph names");
            for (size_t i = 0; i < st.out.size(); i++) {
                if (st.out[i] < 0) continue;
                owned[(size_t)st.out[i]].reset(new Tensor(std::move(out[i])));
                val[(size_t)st.out[i]] = owned[(size_t)st.out[i]].get();
            }
            // a view keeps its base alive: the base's count was raised by one at compile time for exactly this reason
            for (int id : st.release_after) {
                if (--pending[(size_t)id] == 0) { owned[(size_t)id].reset(); }
            }
        }
        std::vector<Tensor> result;
        std::set<int> moved;
        for (auto &o : outputs_) {
            const int id = ids_.at(o.name);
            if (!val[(size_t)id]) throw GraphError("run: output " + o.name + " is not produced by an operator");
            // a graph output that is a graph input or an initializer (not owned by this run), one that is listed twice, and a
            // view (its storage belongs to a value that dies with this run) are handed out as copies; so is whatever else does not own its storage -- the
            // result of a host-evaluated step (Shape(x), shape arithmetic) aliases that step's cached device copy, which the next runs share and evict
            if (!owned[(size_t)id] || moved.count(id) || view_values_.count(id) || !owned[(size_t)id]->owns()) {
                const Tensor &v = moved.count(id) ? result[(size_t)std::distance(outputs_.begin(), std::find_if(outputs_.begin(), outputs_.end(), [&](const onnx::ValueInfo &x) { return x.name == o.name; }))]
                                                  : *val[(size_t)id];
                Tensor copy(ctx_, v.shape(), v.dtype());
                if (v.bytes()) ctx_.check(rten_hip_memcpy_d2d(ctx_.raw(), copy.ptr(), v.ptr(), v.bytes()));
                result.push_back(std::move(copy));
            } else {
                result.push_back(std::move(*owned[(size_t)id]));
                moved.insert(id);
            }
        }
        return result;
    }

    // What a GRU / LSTM node asks for, read as onnx_registry.rs:1214-1226,1306-1370 reads it: activations other than the defaults, activation_alpha / _beta,
    // clip != 0, layout != 0 and input_forget != 0 are load errors that name the node; so are GRU's linear_before_reset=0 (the operator refuses it,
    // rnn.rs:153-158: no point in loading such a model), a peephole input, and a sequence_lens input (the reference reads it and ignores it: refusing is the
    // safe reading, and exporters leave it empty for unpacked input).  Needs no device.
    struct RnnNode {
        bool lstm = false;
        RnnDirection direction = RnnDirection::Forward;
        int64_t hidden_size = 0;
        unsigned output_mask = 0; // bit i: output i is named
    };
    static RnnNode read_rnn_node(const onnx::Node &n, const std::string &label) {
        const std::string kind = n.op_type, where = kind + " " + label + ": ";
        RnnNode a;
        a.lstm = kind == "LSTM";
        if (!n.attr("hidden_size")) throw GraphError(where + "the hidden_size attribute is missing");
        a.hidden_size = n.get_int("hidden_size", 0);
        if (const onnx::Attr *d = n.attr("direction")) {
            if (d->s == "forward") a.direction = RnnDirection::Forward;
            else if (d->s == "reverse") a.direction = RnnDirection::Reverse;
            else if (d->s == "bidirectional") a.direction = RnnDirection::Bidirectional;
            else throw GraphError(where + "direction=\"" + d->s + "\" is not supported");
        }
        const size_t dirs = a.direction == RnnDirection::Bidirectional ? 2 : 1;
        for (const char *nm : {"activation_alpha", "activation_beta"})
            if (const onnx::Attr *p = n.attr(nm)) if (!p->floats.empty()) throw GraphError(where + nm + " is not supported");
        if (const onnx::Attr *p = n.attr("activations")) {
            static const std::vector<std::string> gru_acts = {"Sigmoid", "Tanh"}, lstm_acts = {"Sigmoid", "Tanh", "Tanh"};
            const std::vector<std::string> &defaults = a.lstm ? lstm_acts : gru_acts;
            bool ok = p->strings.empty() || p->strings.size() == defaults.size() * dirs;
            for (size_t i = 0; ok && i < p->strings.size(); i++) ok = p->strings[i] == defaults[i % defaults.size()];
            if (!ok) throw GraphError(where + "activations other than the defaults are not supported");
        }
        if (n.get_float("clip", 0.f) != 0.f) throw GraphError(where + "clip is not supported");
        if (n.get_int("layout", 0) != 0) throw GraphError(where + "layout=" + std::to_string(n.get_int("layout", 0)) + " is not supported");
        if (a.lstm && n.get_int("input_forget", 0) != 0) throw GraphError(where + "input_forget is not supported");
        if (!a.lstm && n.get_int("linear_before_reset", 0) == 0) throw GraphError(where + "`linear_before_reset=0` is not supported");
        if (n.inputs.size() > 4 && !n.inputs[4].empty()) throw GraphError(where + "a sequence_lens input is not supported (the reference ignores it)");
        if (a.lstm && n.inputs.size() > 7 && !n.inputs[7].empty()) throw GraphError(where + "a peephole input (P) is not supported");
        for (size_t k = 0; k < n.outputs.size() && k < (a.lstm ? 3u : 2u); k++) if (!n.outputs[k].empty()) a.output_mask |= 1u << k;
        return a;
    }

    // What an InstanceNormalization / BatchNormalization / LogSoftmax node asks for, read as onnx_registry.rs:830-842,1254-1257,1289-1292 reads it.
    // BatchNormalization: training_mode != 0 and spatial != 1 are load errors that name the node, momentum is ignored, and a named output beyond Y
    // (running_mean, running_var, saved_mean, saved_var: training only, norm.rs:249-256) is refused like MaxPool's Indices.  Needs no device.
    // What the loader reads from, and refuses about, a Pad / Pow node (make_pad_step / make_math_step; rten_hip_run --parse-only runs the same checks without a
    // device).  `m` = the canonical model: an operand is a constant when an initializer carries its name, device data when it is a graph input.
    struct PadNode {
        int mode = RTEN_HIP_PAD_CONSTANT;
        std::string mode_name = "constant";
        bool attr_form = false;       // before opset 11: the pads / value attributes (onnx_registry.rs:1545-1552)
        std::vector<int64_t> pads;
        float value = 0.f;
    };
    static const onnx::TensorProto *initializer_named(const onnx::Model &m, const std::string &v) {
        for (auto &t : m.initializers) if (t.name == v) return &t;
        return nullptr;
    }
    static const onnx::ValueInfo *graph_input_named(const onnx::Model &m, const std::string &v) {
        for (auto &gi : m.inputs) if (gi.name == v && !initializer_named(m, v)) return &gi;
        return nullptr;
    }
    static PadNode read_pad_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "Pad " + label + ": ";
        PadNode a;
        if (const onnx::Attr *ma = n.attr("mode")) if (!ma->s.empty()) a.mode_name = ma->s;
        a.mode = pad_mode_of(a.mode_name);
        if (a.mode < 0) throw GraphError(where + "mode \"" + a.mode_name + "\" is not supported (constant, reflect, edge, wrap)");
        if (n.inputs.size() > 3 && !n.inputs[3].empty()) throw GraphError(where + "Pad operator does not yet support `axes` input");
        if (const onnx::Attr *pa = n.attr("pads")) { a.attr_form = true; a.pads = pa->ints; a.value = n.get_float("value", 0.f); return a; }
        if (n.inputs.size() < 2 || n.inputs[1].empty()) throw GraphError(where + "the pads input is missing");
        if (graph_input_named(m, n.inputs[1]))
            throw GraphError(where + "pads must be a constant or computable from the input shapes (it is the graph input \"" + n.inputs[1] + "\", device data at run time)");
        if (n.inputs.size() > 2 && !n.inputs[2].empty() && graph_input_named(m, n.inputs[2]))
            throw GraphError(where + "constant_value must be a constant or computable from the input shapes (it is the graph input \"" + n.inputs[2] + "\", device data at run time)");
        return a;
    }
    // Pow: the reference's int32-base forms are not built; a base whose element type the model states (an initializer or a graph input) is refused at load
    static void check_pow_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        if (n.inputs.empty()) return;
        int et = 0;
        if (const onnx::TensorProto *t = initializer_named(m, n.inputs[0])) et = t->data_type;
        else if (const onnx::ValueInfo *gi = graph_input_named(m, n.inputs[0])) et = gi->elem_type;
        if (et == onnx::INT32 || et == onnx::INT64) throw GraphError("Pow " + label + ": an int32 base is not supported by the device path (float32 base and exponent only)");
    }
    // The Reduce* kinds make_reduce_step takes beyond Sum / Mean / Max / Min, as the RTEN_HIP_REDUCE_* kernel each runs; -1: not one of them
    static int reduce_family_kind(const std::string &k) {
        static const std::map<std::string, int> kinds = {{"ReduceL1", RTEN_HIP_REDUCE_L1}, {"ReduceSumSquare", RTEN_HIP_REDUCE_SUM_SQUARE}, {"ReduceL2", RTEN_HIP_REDUCE_L2},
                                                         {"ReduceLogSum", RTEN_HIP_REDUCE_LOG_SUM}, {"ReduceLogSumExp", RTEN_HIP_REDUCE_LOG_SUM_EXP}, {"ReduceProd", RTEN_HIP_REDUCE_PROD}};
        auto it = kinds.find(k);
        return it == kinds.end() ? -1 : it->second;
    }
    // What the loader reads from, and refuses about, an LpNormalization node (onnx_registry.rs:1284-1287: axis defaults to -1, p to 2; any other p is the
    // operator's UnsupportedValue, norm.rs:644-646: no point in loading such a model).  Needs no device; rten_hip_run --parse-only calls it too.
    struct LpNormNode { int axis = -1, p = 2; };
    static LpNormNode read_lp_norm_node(const onnx::Node &n, const std::string &label) {
        LpNormNode a;
        a.axis = (int)n.get_int("axis", -1);
        const int64_t p = n.get_int("p", 2);
        if (p != 1 && p != 2) throw GraphError("LpNormalization " + label + ": p = " + std::to_string(p) + " is not supported (`p` must be 1 or 2)");
        a.p = (int)p;
        return a;
    }
    // What the loader reads from, and refuses about, the decoder-block nodes (make_decoder_step): RMSNormalization and SimplifiedLayerNormalization in ai.onnx
    // (onnx_registry.rs:1584-1590,1905-1911: axis defaults to -1, epsilon to the operator's 1e-5, stash_type must be 1), SkipLayerNormalization and
    // SkipSimplifiedLayerNormalization in com.microsoft (onnx_registry.rs:1918-1933: epsilon is required) and the two RotaryEmbedding operators
    // (onnx_registry.rs:1815-1847).  The skip forms compute output 0 and output 3 (the sum): the reference fills outputs 1 and 2 (mean, inv_std_var:
    // training outputs) with scalar zeros, here a node whose output 1 or 2 is READ -- by a node or as a graph output -- is refused; named but unread is fine.
    // An input whose element type the model states (an initializer or a graph input) must be float32 (position_ids: int32 / int64).  Needs no device;
    // rten_hip_run --parse-only calls it too.
    static bool is_decoder_node(const onnx::Node &n) {
        const bool std_domain = n.domain.empty() || n.domain == "ai.onnx";
        if (std_domain) return n.op_type == "RMSNormalization" || n.op_type == "SimplifiedLayerNormalization" || n.op_type == "RotaryEmbedding";
        return n.domain == "com.microsoft" && (n.op_type == "SkipLayerNormalization" || n.op_type == "SkipSimplifiedLayerNormalization" || n.op_type == "RotaryEmbedding");
    }
    static bool value_is_read(const onnx::Model &m, const std::string &v) {
        if (v.empty()) return false;
        for (auto &o : m.outputs) if (o.name == v) return true;
        for (auto &nd : m.nodes) for (auto &s : nd.inputs) if (s == v) return true;
        return false;
    }
    // The RMSNormalization / SimplifiedLayerNormalization node that the Add at `add` fuses with (make_add_norm_step; off under --no-fuse): it reads the sum as
    // its input, normalises the last axis (axis -1), and its scale exists before the Add runs.  -1: none.  From the model alone, so --parse-only can say it.
    static long add_rms_consumer(const onnx::Model &m, size_t add) {
        const onnx::Node &a = m.nodes[add];
        if (a.op_type != "Add" || !(a.domain.empty() || a.domain == "ai.onnx") || a.inputs.size() != 2 || a.outputs.empty()) return -1;
        const std::string &sum = a.outputs[0];
        for (size_t u = 0; u < m.nodes.size(); u++) {
            const onnx::Node &c = m.nodes[u];
            if (!(c.domain.empty() || c.domain == "ai.onnx") || (c.op_type != "RMSNormalization" && c.op_type != "SimplifiedLayerNormalization")) continue;
            if (c.inputs.size() != 2 || c.inputs[0] != sum || c.inputs[1] == sum || c.get_int("axis", -1) != -1 || c.get_int("stash_type", 1) != 1) continue;
            bool ready = true;
            for (size_t q = add; q < m.nodes.size(); q++) for (auto &o : m.nodes[q].outputs) if (o == c.inputs[1]) ready = false;
            if (ready) return (long)u;
        }
        return -1;
    }
    struct DecoderNode {
        bool contrib = false, rotary = false, skip = false, rms = false; // rms: the root-mean-square statistic (every normalisation here but SkipLayerNormalization)
        int axis = -1;
        std::optional<float> epsilon;
        bool want_sum = false; // a skip form whose output 3 is read
        bool interleaved = false;
        int64_t num_heads = 0, rotary_embedding_dim = 0;
    };
    static DecoderNode read_decoder_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        DecoderNode a;
        a.contrib = n.domain == "com.microsoft";
        a.rotary = n.op_type == "RotaryEmbedding";
        a.skip = a.contrib && !a.rotary;
        a.rms = !a.rotary && n.op_type != "SkipLayerNormalization";
        const std::string where = (a.contrib ? "com.microsoft." : "") + n.op_type + " " + label + ": ";
        auto stated = [&](const std::string &v) {
            if (const onnx::TensorProto *t = initializer_named(m, v)) return t->data_type;
            if (const onnx::ValueInfo *gi = graph_input_named(m, v)) return gi->elem_type;
            return 0;
        };
        auto floats = [&](std::initializer_list<size_t> which) {
            for (size_t i : which) {
                if (i >= n.inputs.size() || n.inputs[i].empty()) continue;
                const int et = stated(n.inputs[i]);
                if (et != 0 && et != onnx::FLOAT) throw GraphError(where + "input " + std::to_string(i) + " (\"" + n.inputs[i] + "\") has element type " + std::to_string(et) + ": float32 only");
            }
        };
        auto needs = [&](size_t count, const char *what) {
            for (size_t i = 0; i < count; i++) if (i >= n.inputs.size() || n.inputs[i].empty()) throw GraphError(where + "the " + what + " inputs are required");
        };
        if (a.rotary) {
            a.interleaved = n.get_int("interleaved", 0) != 0;
            a.num_heads = n.get_int("num_heads", 0);
            a.rotary_embedding_dim = n.get_int("rotary_embedding_dim", 0);
            if (a.num_heads < 0 || a.rotary_embedding_dim < 0) throw GraphError(where + "num_heads and rotary_embedding_dim must not be negative");
            refuse_extra_inputs(n, 4, where);
            needs(a.contrib ? 4 : 3, a.contrib ? "input, position_ids, cos_cache and sin_cache" : "X, cos_cache and sin_cache");
            if (a.contrib) floats({0, 2, 3}); else floats({0, 1, 2});
            const size_t ids = a.contrib ? 1 : 3;
            if (ids < n.inputs.size() && !n.inputs[ids].empty()) {
                const int et = stated(n.inputs[ids]);
                if (et != 0 && et != onnx::INT32 && et != onnx::INT64) throw GraphError(where + "position_ids (\"" + n.inputs[ids] + "\") has element type " + std::to_string(et) + ": int32 / int64 only");
            }
            return a;
        }
        if (a.skip) {
            const onnx::Attr *eps = n.attr("epsilon");
            if (!eps) throw GraphError(where + "the epsilon attribute is missing");
            a.epsilon = eps->f;
            refuse_extra_inputs(n, a.rms ? 4 : 5, where);
            needs(3, "input, skip and gamma");
            floats({0, 1, 2, 3, 4});
            static const char *slot[] = {"", "mean", "inv_std_var"};
            for (size_t k = 1; k <= 2; k++)
                if (k < n.outputs.size() && value_is_read(m, n.outputs[k]))
                    throw GraphError(where + "output " + std::to_string(k) + " (" + slot[k] + ", \"" + n.outputs[k] + "\") is read, but only output 0 and output 3 (the sum) are computed");
            if (n.outputs.size() > 4) throw GraphError(where + "has at most 4 outputs (it names " + std::to_string(n.outputs.size()) + ")");
            a.want_sum = n.outputs.size() > 3 && value_is_read(m, n.outputs[3]);
            return a;
        }
        a.axis = (int)n.get_int("axis", -1);
        if (const onnx::Attr *eps = n.attr("epsilon")) a.epsilon = eps->f;
        const int64_t stash = n.get_int("stash_type", 1);
        if (stash != 1) throw GraphError(where + "stash_type = " + std::to_string(stash) + " is not supported (the statistic is computed in float32: stash_type must be 1)");
        refuse_extra_inputs(n, 2, where);
        needs(2, "X and scale");
        floats({0, 1});
        return a;
    }
    // What the loader reads from, and refuses about, a com.microsoft GroupQueryAttention node (make_gqa_step; attributes and their defaults:
    // onnx_registry.rs:1467-1492 -- num_heads and kv_num_heads are required, a non-positive local_window_size disables the window).  Refused by node name:
    // smooth_softmax, a head_sink input, softcap != 0 (the reference calls libm's tanh there: not reproducible), inputs 12-15 (quantisation scales, q / k
    // norm weights), output 3 (output_qk), and an input whose stated element type is not float32 (seqlens_k, total_sequence_length, position_ids: int32 /
    // int64).  Needs no device; rten_hip_run --parse-only calls it too.
    static bool is_gqa_node(const onnx::Node &n) { return n.domain == "com.microsoft" && n.op_type == "GroupQueryAttention"; }
    struct GqaNode {
        int64_t num_heads = 0, kv_num_heads = 0, local_window_size = -1;
        std::optional<float> scale;
        bool do_rotary = false, rotary_interleaved = false, packed = false, want_present = false;
    };
    static GqaNode read_gqa_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "com.microsoft.GroupQueryAttention " + label + ": ";
        GqaNode a;
        if (!n.attr("num_heads") || !n.attr("kv_num_heads")) throw GraphError(where + "the num_heads and kv_num_heads attributes are required");
        a.num_heads = n.get_int("num_heads", 0);
        a.kv_num_heads = n.get_int("kv_num_heads", 0);
        if (a.num_heads <= 0 || a.kv_num_heads <= 0) throw GraphError(where + "num_heads and kv_num_heads must be positive");
        if (a.num_heads % a.kv_num_heads != 0) throw GraphError(where + "num_heads must be a multiple of kv_num_heads");
        if (const onnx::Attr *sc = n.attr("scale")) a.scale = sc->f;
        a.do_rotary = n.get_int("do_rotary", 0) != 0;
        a.rotary_interleaved = n.get_int("rotary_interleaved", 0) != 0;
        a.local_window_size = n.get_int("local_window_size", -1);
        if (n.get_int("smooth_softmax", 0) != 0) throw GraphError(where + "smooth_softmax is not supported");
        if (n.get_float("softcap", 0.f) != 0.f) throw GraphError(where + "softcap != 0 is not supported");
        auto present = [&](size_t i) { return i < n.inputs.size() && !n.inputs[i].empty(); };
        if (present(11)) throw GraphError(where + "the head_sink input (\"" + n.inputs[11] + "\") is not supported");
        for (size_t i = 12; i < n.inputs.size(); i++)
            if (present(i)) throw GraphError(where + "input " + std::to_string(i) + " (\"" + n.inputs[i] + "\") is not supported (inputs 12-15: quantisation scales and q / k norm weights)");
        if (n.outputs.size() > 3 && !n.outputs[3].empty()) throw GraphError(where + "output 3 (output_qk, \"" + n.outputs[3] + "\") is not supported");
        if (!present(0) || !present(5) || !present(6)) throw GraphError(where + "the query, seqlens_k and total_sequence_length inputs are required");
        if (present(1) != present(2)) throw GraphError(where + "key and value must both be present or both absent");
        if (present(3) != present(4)) throw GraphError(where + "past_key and past_value must both be present or both absent");
        if (a.do_rotary && (!present(7) || !present(8))) throw GraphError(where + "cos_cache and sin_cache are required when do_rotary is set");
        a.packed = !present(1);
        auto stated = [&](const std::string &v) {
            if (const onnx::TensorProto *t = initializer_named(m, v)) return t->data_type;
            if (const onnx::ValueInfo *gi = graph_input_named(m, v)) return gi->elem_type;
            return 0;
        };
        for (size_t i : {0, 1, 2, 3, 4, 7, 8, 10}) {
            if (!present(i)) continue;
            const int et = stated(n.inputs[i]);
            if (et != 0 && et != onnx::FLOAT) throw GraphError(where + "input " + std::to_string(i) + " (\"" + n.inputs[i] + "\") has element type " + std::to_string(et) + ": float32 only");
        }
        for (size_t i : {5, 6, 9}) {
            if (!present(i)) continue;
            const int et = stated(n.inputs[i]);
            if (et != 0 && et != onnx::INT32 && et != onnx::INT64) throw GraphError(where + "input " + std::to_string(i) + " (\"" + n.inputs[i] + "\") has element type " + std::to_string(et) + ": int32 / int64 only");
        }
        for (size_t k = 1; k <= 2; k++) a.want_present = a.want_present || (k < n.outputs.size() && value_is_read(m, n.outputs[k]));
        return a;
    }
    // What the loader refuses about a Reduce* node of reduce_family_kind: axes that are neither an attribute nor a constant input are found when the plan
    // is built (read_reduce_attrs); here, without a device, an axes input that is a graph input (device data at run time).
    static void check_reduce_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        if (n.inputs.size() > 1 && !n.inputs[1].empty() && graph_input_named(m, n.inputs[1]))
            throw GraphError(n.op_type + " " + label + ": the axes input must be a constant (it is the graph input \"" + n.inputs[1] + "\", device data at run time)");
    }
    // What the loader reads from, and refuses about, a GridSample node (onnx_registry.rs:1203-1212): align_corners defaults to 0; mode must be
    // "bilinear" (opset 16) or "linear" (opset 20), padding_mode "zeros".  Needs no device; rten_hip_run --parse-only calls it too.
    struct GridSampleNode { bool align_corners = false; };
    static GridSampleNode read_grid_sample_node(const onnx::Node &n, const std::string &label) {
        GridSampleNode a;
        a.align_corners = n.get_int("align_corners", 0) != 0;
        if (const onnx::Attr *mode = n.attr("mode"))
            if (mode->s != "bilinear" && mode->s != "linear") throw GraphError("GridSample " + label + ": mode=\"" + mode->s + "\" is not supported (bilinear / linear only)");
        if (const onnx::Attr *pad = n.attr("padding_mode"))
            if (pad->s != "zeros") throw GraphError("GridSample " + label + ": padding_mode=\"" + pad->s + "\" is not supported (zeros only)");
        return a;
    }
    // ... and a DepthToSpace node (onnx_registry.rs:1094-1107): mode "DCR" (the default) or "CRD"; blocksize is required and must fit the
    // reference's u32 (0 is read, and refused by the operator: "`block_size` must be > 0").
    struct DepthToSpaceNode { int64_t block_size = 0; DepthToSpaceMode mode = DepthToSpaceMode::DepthColumnRow; };
    static DepthToSpaceNode read_depth_to_space_node(const onnx::Node &n, const std::string &label) {
        DepthToSpaceNode a;
        if (const onnx::Attr *mode = n.attr("mode")) {
            if (mode->s == "CRD") a.mode = DepthToSpaceMode::ColumnRowDepth;
            else if (mode->s != "DCR") throw GraphError("DepthToSpace " + label + ": mode=\"" + mode->s + "\" is not supported (DCR / CRD only)");
        }
        const onnx::Attr *bs = n.attr("blocksize");
        if (!bs) throw GraphError("DepthToSpace " + label + ": the blocksize attribute is missing");
        if (bs->i < 0 || bs->i > 0xffffffffll) throw GraphError("DepthToSpace " + label + ": blocksize " + std::to_string(bs->i) + " is out of range");
        a.block_size = bs->i;
        return a;
    }
    // What the loader reads from, and refuses about, a CumSum / GatherElements / Trilu / Tile node (make_index_step; onnx_registry.rs:1056-1060 and the
    // operators' max_inputs).  The axis of CumSum, k of Trilu and the repeats of Tile are host values at run time -- constants or shape arithmetic -- so one
    // that is a graph input (device data) is refused here, by node name; any other device-computed one is refused by the step when it runs.  Needs no
    // device; rten_hip_run --parse-only calls them too.
    static void refuse_device_operand(const onnx::Model &m, const onnx::Node &n, size_t i, const std::string &where, const char *what) {
        if (n.inputs.size() > i && !n.inputs[i].empty() && graph_input_named(m, n.inputs[i]))
            throw GraphError(where + what + " must be a constant or computable from the input shapes (it is the graph input \"" + n.inputs[i] + "\", device data at run time)");
    }
    static void refuse_extra_inputs(const onnx::Node &n, size_t max, const std::string &where) {
        if (n.inputs.size() > max) throw GraphError(where + "takes at most " + std::to_string(max) + " inputs (it has " + std::to_string(n.inputs.size()) + ")");
    }
    struct CumSumNode { bool exclusive = false, reverse = false; };
    static CumSumNode read_cumsum_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "CumSum " + label + ": ";
        CumSumNode a;
        a.exclusive = n.get_int("exclusive", 0) != 0;
        a.reverse = n.get_int("reverse", 0) != 0;
        refuse_extra_inputs(n, 2, where);
        if (n.inputs.size() < 2 || n.inputs[1].empty()) throw GraphError(where + "the axis input is missing");
        refuse_device_operand(m, n, 1, where, "axis");
        return a;
    }
    struct GatherElementsNode { int axis = 0; };
    static GatherElementsNode read_gather_elements_node(const onnx::Node &n, const std::string &label) {
        GatherElementsNode a;
        a.axis = (int)n.get_int("axis", 0);
        refuse_extra_inputs(n, 2, "GatherElements " + label + ": ");
        return a;
    }
    struct TriluNode { bool upper = true; };
    static TriluNode read_trilu_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "Trilu " + label + ": ";
        TriluNode a;
        a.upper = n.get_int("upper", 1) != 0;
        refuse_extra_inputs(n, 2, where);
        refuse_device_operand(m, n, 1, where, "k");
        return a;
    }
    static void read_tile_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "Tile " + label + ": ";
        refuse_extra_inputs(n, 2, where);
        if (n.inputs.size() < 2 || n.inputs[1].empty()) throw GraphError(where + "the repeats input is missing");
        refuse_device_operand(m, n, 1, where, "repeats");
    }
    // What the loader reads from, and refuses about, a NonMaxSuppression node (make_nms_step; onnx_registry.rs and the operator's max_inputs): an unknown
    // center_point_box, more than 5 inputs, fewer than 2, and a graph input (device data at run time) in place of one of the three scalars.
    struct NmsNode { int center_point_box = 0; bool has_max = false, has_iou = false, has_score = false; };
    static NmsNode read_nms_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "NonMaxSuppression " + label + ": ";
        NmsNode a;
        const int64_t cpb = n.get_int("center_point_box", 0);
        if (cpb != 0 && cpb != 1) throw GraphError(where + "center_point_box " + std::to_string(cpb) + " is not 0 ([y1, x1, y2, x2]) or 1 ([cx, cy, w, h])");
        a.center_point_box = (int)cpb;
        refuse_extra_inputs(n, 5, where);
        if (n.inputs.size() < 2 || n.inputs[0].empty() || n.inputs[1].empty()) throw GraphError(where + "the boxes or scores input is missing");
        refuse_device_operand(m, n, 2, where, "max_output_boxes_per_class");
        refuse_device_operand(m, n, 3, where, "iou_threshold");
        refuse_device_operand(m, n, 4, where, "score_threshold");
        a.has_max = n.inputs.size() > 2 && !n.inputs[2].empty();
        a.has_iou = n.inputs.size() > 3 && !n.inputs[3].empty();
        a.has_score = n.inputs.size() > 4 && !n.inputs[4].empty();
        return a;
    }
    // What the loader reads from, and refuses about, a DFT / STFT node (make_fft_step; onnx_registry.rs:1063-1079,1991-1994 and the operators' max_inputs).
    // inverse and onesided default to 0 for DFT, onesided to 1 for STFT.  DFT's axis: the `axis` attribute where the node has one; else 1 before opset 20; else
    // the optional third input, default -2.  dft_length, axis, frame_step and frame_length are host values at run time -- constants or shape arithmetic -- so
    // one that is a graph input (device data) is refused here, by node name; any other device-computed one is refused by the step when it runs.  Needs no
    // device; rten_hip_run --parse-only calls them too.
    struct DftNode { bool inverse = false, onesided = false, axis_fixed = false; int64_t axis = -2; };
    static DftNode read_dft_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "DFT " + label + ": ";
        DftNode a;
        a.inverse = n.get_int("inverse", 0) != 0;
        a.onesided = n.get_int("onesided", 0) != 0;
        const int64_t none = INT64_MIN;
        const int64_t attr = n.get_int("axis", none);
        if (attr != none) { a.axis_fixed = true; a.axis = attr; }
        else if (m.opset < 20) { a.axis_fixed = true; a.axis = 1; }
        refuse_extra_inputs(n, 3, where);
        if (n.inputs.empty() || n.inputs[0].empty()) throw GraphError(where + "the input is missing");
        refuse_device_operand(m, n, 1, where, "dft_length");
        refuse_device_operand(m, n, 2, where, "axis");
        return a;
    }
    struct StftNode { bool onesided = true, has_window = false, has_frame_length = false; };
    static StftNode read_stft_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = "STFT " + label + ": ";
        StftNode a;
        a.onesided = n.get_int("onesided", 1) != 0;
        refuse_extra_inputs(n, 4, where);
        if (n.inputs.size() < 2 || n.inputs[0].empty() || n.inputs[1].empty()) throw GraphError(where + "the signal or frame_step input is missing");
        refuse_device_operand(m, n, 1, where, "frame_step");
        refuse_device_operand(m, n, 3, where, "frame_length");
        a.has_window = n.inputs.size() > 2 && !n.inputs[2].empty();
        a.has_frame_length = n.inputs.size() > 3 && !n.inputs[3].empty();
        if (!a.has_window && !a.has_frame_length) throw GraphError(where + "Either frame_length or window must be set");
        return a;
    }
    static bool is_index_kind(const std::string &k) { return k == "CumSum" || k == "GatherElements" || k == "Trilu" || k == "Tile"; }
    static bool is_math_kind(const std::string &k) {
        static const std::set<std::string> kinds = {"Neg", "Abs", "Sign", "Floor", "Ceil", "Round", "Sqrt", "Reciprocal", "Exp", "Log", "Softplus", "Pow", "PRelu", "Min", "Max", "Sum", "Mean"};
        return kinds.count(k) != 0;
    }
    // hostable: evaluated on the host when every operand is a host value
    static bool is_hostable_math_kind(const std::string &k) {
        static const std::set<std::string> kinds = {"Neg", "Abs", "Sign", "Floor", "Ceil", "Round", "Sqrt", "Reciprocal", "Min", "Max"};
        return kinds.count(k) != 0;
    }
    // What the loader reads from, and refuses about, a QuantizeLinear / DequantizeLinear node (onnx_registry.rs:1081-1092,1560-1582: axis defaults to -1 for
    // QuantizeLinear and to 1 for DequantizeLinear).  Needs no device; make_qdq_step and rten_hip_run --parse-only both call it.
    struct QdqNode {
        bool quantize = false;
        int axis = 0;
        std::optional<DType> output_dtype; // QuantizeLinear: the output_dtype attribute (UINT8 / INT8) when it is given
        bool has_zero_point = false;
    };
    static QdqNode read_qdq_node(const onnx::Model &m, const onnx::Node &n, const std::string &label) {
        const std::string where = n.op_type + " " + label + ": ";
        QdqNode a;
        a.quantize = n.op_type == "QuantizeLinear";
        a.axis = (int)n.get_int("axis", a.quantize ? -1 : 1);
        a.has_zero_point = n.inputs.size() > 2 && !n.inputs[2].empty();
        if (n.get_int("block_size", 0) != 0) throw GraphError(where + "block_size " + std::to_string(n.get_int("block_size", 0)) + ": blocked quantization is not supported");
        if (n.get_int("saturate", 1) != 1) throw GraphError(where + "saturate = " + std::to_string(n.get_int("saturate", 1)) + " is not supported (float8 outputs only)");
        if (n.get_int("precision", 0) != 0) throw GraphError(where + "precision = " + std::to_string(n.get_int("precision", 0)) + " is not supported");
        const int64_t od = n.get_int("output_dtype", 0);
        if (!a.quantize) {
            if (od != 0) throw GraphError(where + "output_dtype = " + std::to_string(od) + " is not supported (the output is float32)");
            return a;
        }
        if (od != 0 && od != onnx::UINT8 && od != onnx::INT8) throw GraphError(where + "output_dtype = " + std::to_string(od) + " is not supported (uint8 or int8)");
        if (od != 0) a.output_dtype = od == onnx::UINT8 ? DType::U8 : DType::I8;
        if (!a.has_zero_point && od == 0) throw GraphError(where + "neither a zero-point input nor output_dtype gives the output type");
        return a;
    }
    // The DequantizeLinear that a QuantizeLinear (node i of the canonical model) forms one round-trip step with, or -1: the quantised value has exactly one
    // reader, a DequantizeLinear taking it as data, and is not a graph output; both nodes take constant scales and zero points with bitwise equal values (both
    // or neither have a zero point) and the same quantisation axis.  A per-axis pair whose two `axis` attributes differ is left alone even where they would
    // resolve to the same dim for the rank met at run time (the rank is not known here).
    static long qdq_pair_partner(const onnx::Model &m, size_t i) {
        const onnx::Node &q = m.nodes[i];
        if (q.op_type != "QuantizeLinear" || q.inputs.size() < 2 || q.outputs.empty() || !(q.domain.empty() || q.domain == "ai.onnx")) return -1;
        const std::string &v = q.outputs[0];
        for (auto &o : m.outputs) if (o.name == v) return -1;
        long reader = -1;
        for (size_t j = 0; j < m.nodes.size(); j++)
            for (auto &in : m.nodes[j].inputs)
                if (in == v) { if (reader >= 0) return -1; reader = (long)j; }
        if (reader < 0) return -1;
        const onnx::Node &d = m.nodes[(size_t)reader];
        if (d.op_type != "DequantizeLinear" || d.inputs.size() < 2 || d.inputs[0] != v || !(d.domain.empty() || d.domain == "ai.onnx")) return -1;
        auto same_const = [&](const std::string &a, const std::string &b) {
            const onnx::TensorProto *ta = initializer_named(m, a), *tb = initializer_named(m, b);
            return ta && tb && ta->data_type == tb->data_type && ta->raw == tb->raw && (ta->len() == 1 || ta->dims == tb->dims);
        };
        if (!same_const(q.inputs[1], d.inputs[1])) return -1;
        const bool qz = q.inputs.size() > 2 && !q.inputs[2].empty(), dz = d.inputs.size() > 2 && !d.inputs[2].empty();
        if (qz != dz || (qz && !same_const(q.inputs[2], d.inputs[2]))) return -1;
        const onnx::TensorProto *sc = initializer_named(m, q.inputs[1]);
        if (sc->data_type != onnx::FLOAT) return -1;
        if (sc->len() != 1 && q.get_int("axis", -1) != d.get_int("axis", 1)) return -1;
        return reader;
    }
    // Constant DequantizeLinear (data, scale and zero point all initializers), evaluated at load as the reference's propagate_constants does: one exact
    // int -> f32 conversion (ties to even above 2^24, Rust's `as f32`) and one IEEE multiply per element -- the kernel's bits.  Errors name the node.
    static onnx::TensorProto fold_dequantize(const onnx::Node &n, const onnx::TensorProto &x, const onnx::TensorProto &scale, const onnx::TensorProto *zp) {
        const std::string where = "DequantizeLinear " + label_of(n) + ": ";
        read_qdq_node(onnx::Model(), n, label_of(n));
        if (scale.data_type != onnx::FLOAT) throw GraphError(where + "the scale must be float32");
        if (x.data_type != onnx::UINT8 && x.data_type != onnx::INT8 && x.data_type != onnx::INT32) throw GraphError(where + "the input must be uint8, int8 or int32");
        if (zp && zp->data_type != x.data_type) throw GraphError(where + "the zero point must have the input's type");
        const size_t esz = x.data_type == onnx::INT32 ? 4 : 1;
        if (x.raw.size() != (size_t)x.len() * esz || scale.raw.size() != (size_t)scale.len() * 4 || (zp && zp->raw.size() != (size_t)zp->len() * esz))
            throw GraphError(where + "an initializer's data size does not match its dims");
        QdqGeometry g;
        try { g = qdq_geometry(x.dims, scale.dims, zp ? &zp->dims : nullptr, (int)n.get_int("axis", 1), true); }
        catch (const OpError &e) { throw GraphError(where + e.msg); }
        auto elem = [esz](const onnx::TensorProto &t, int64_t i) -> int32_t {
            if (esz == 4) { int32_t v; std::memcpy(&v, t.raw.data() + 4 * i, 4); return v; }
            return t.data_type == onnx::UINT8 ? (int32_t)(uint8_t)t.raw[(size_t)i] : (int32_t)(int8_t)t.raw[(size_t)i];
        };
        onnx::TensorProto y;
        y.name = n.outputs.at(0);
        y.dims = x.dims;
        y.data_type = onnx::FLOAT;
        y.raw.resize((size_t)x.len() * 4);
        int64_t at = 0;
        for (int64_t o = 0; o < g.outer; o++)
            for (int64_t c = 0; c < g.channels; c++) {
                float s;
                std::memcpy(&s, scale.raw.data() + 4 * c, 4);
                const int32_t z = zp ? elem(*zp, c) : 0;
                for (int64_t k = 0; k < g.inner; k++, at++) {
                    const float v = (float)(int32_t)((uint32_t)elem(x, at) - (uint32_t)z) * s;
                    std::memcpy(&y.raw[(size_t)at * 4], &v, 4);
                }
            }
        return y;
    }
    struct NormNode {
        std::optional<float> epsilon; // absent: the operator's default (1e-5)
        int axis = -1;                // LogSoftmax
    };
    static NormNode read_norm_node(const onnx::Node &n, const std::string &label) {
        const std::string kind = n.op_type, where = kind + " " + label + ": ";
        NormNode a;
        if (n.attr("epsilon")) a.epsilon = n.get_float("epsilon", 1e-5f);
        if (kind == "BatchNormalization") {
            if (n.get_int("training_mode", 0) != 0) throw GraphError(where + "training_mode=" + std::to_string(n.get_int("training_mode", 0)) + " is not supported");
            if (n.get_int("spatial", 1) != 1) throw GraphError(where + "spatial=" + std::to_string(n.get_int("spatial", 1)) + " is not supported");
            static const char *outs[] = {"Y", "running_mean", "running_var", "saved_mean", "saved_var"};
            for (size_t k = 1; k < n.outputs.size(); k++)
                if (!n.outputs[k].empty()) throw GraphError(where + "the " + (k < 5 ? outs[k] : "extra") + " output is not supported");
        } else if (kind == "LogSoftmax") a.axis = (int)n.get_int("axis", -1);
        return a;
    }
    // The step name the loader gives norm node `i` of a canonical model when fusion is on -- "InstanceNormalization+Relu", "BatchNormalization+Sigmoid", ... --
    // from the node list alone (the rule of make_norm_step: the sole reader of the output is a Relu or an activation with load-time parameters), for
    // rten_hip_run --parse-only, which has no device to build a plan on.
    static std::string norm_step_name(const onnx::Model &m, size_t i) {
        const onnx::Node &n = m.nodes.at(i);
        const std::string &v = n.outputs.at(0);
        if (n.op_type == "LogSoftmax") return n.op_type;
        for (auto &o : m.outputs) if (o.name == v) return n.op_type;
        const onnx::Node *reader = nullptr;
        size_t readers = 0;
        for (auto &u : m.nodes) for (auto &in : u.inputs) if (in == v) { readers++; reader = &u; }
        if (readers != 1 || reader->inputs[0] != v) return n.op_type;
        if (reader->op_type == "Relu") return n.op_type + "+Relu";
        Activation act;
        auto scalar = [&m](const std::string &name, float &) {
            for (auto &t : m.initializers) if (t.name == name) return t.data_type == 1 && detail::prod(t.dims, 0, t.dims.size()) == 1;
            return false;
        };
        return activation_of(*reader, act, scalar) ? n.op_type + "+" + activation_name(act.kind) : n.op_type;
    }

  private:
    struct I8Conv {
        std::shared_ptr<ConvInteger> op;
        ConvInteger::Staging sg;
        bool to_float = false;
        bool relu = false;
        int tile = -1;         // a launch plan's per-layer workgroup tile for this step's int8 kernel (rten_hip_set_int8_tile; -1 = the backend's rule)
        bool qout_off = false; // the one-launch form was refused once (grid not resident at once): the two-launch sequence from then on
        bool qout_producer = false; // this step also runs its consumer's quantizer (Options::qout): it keeps reading staged codes itself
    };
    struct Step {
        std::string name, kind_name;
        std::vector<int> in, out, release_after;
        std::function<OutputList(Context &, const InputList &)> run;
        bool view = false;
        std::shared_ptr<Conv> conv; // f32 convolution steps: the launch plan is tunable
        std::shared_ptr<GemmPlan> gemm_plan; // MatMul / FusedMatMul / Gemm steps: the same launch plan, applied around the step's GEMM
        std::shared_ptr<I8Conv> i8; // int8 convolution steps: staged-pipeline options are decided after all steps exist
        std::shared_ptr<DynamicQuantizeLinearStaged> dql_staged;
        std::shared_ptr<MaxPool> maxpool; // a max-pool whose output is quantized next can accumulate the quantizer's statistics
        bool removed = false;
        bool batch_coupled = false; // the result for one dim-0 row depends on other rows (no sub-batch chains for such a graph)
        bool reads_back = false;    // the step reads a count back from the device to shape its output (NonMaxSuppression): it synchronises and cannot be captured
        size_t pos = 0; // index of the LAST graph node folded into this step: the step runs where that node stood
        int extra_out = -1; // a value the step produces besides its node's outputs, appended to `out` (the sum of a fused Add -> RMSNormalization that has other readers)
    };

    Context &ctx_;
    Options opt_;
    std::vector<std::string> names_;
    std::map<std::string, int> ids_;
    std::map<int, Tensor> consts_;
    std::vector<std::unique_ptr<Tensor>> packed_; // prepacked conv weights
    std::map<std::string, const Tensor *> packed_of_; // step name -> its prepacked operand (what a sharing graph looks up)
    const Graph *donor_ = nullptr;
    // a constant of this graph: uploaded here, or a non-owning view of the donor's
    void add_const(int id, const std::function<Tensor()> &make) {
        if (donor_) { const Tensor &d = donor_->consts_.at(id); Tensor v = Tensor::view_of(d, d.shape()); v.set_host(d.host_ptr()); consts_.emplace(id, std::move(v)); }
        else consts_.emplace(id, make());
    }
    // the prepacked operand of step `name`: packed here, or the donor's
    const Tensor *packed_for(const std::string &name, const std::function<Tensor()> &pack) {
        if (donor_) { auto it = donor_->packed_of_.find(name); return it == donor_->packed_of_.end() ? nullptr : it->second; }
        Tensor pk = pack();
        if (!pk.len()) return nullptr;
        packed_.emplace_back(new Tensor(std::move(pk)));
        packed_of_[name] = packed_.back().get();
        return packed_.back().get();
    }
    std::vector<Step> steps_;
    std::string runtime_coupled_;
    void note_axis(const std::string &kind, const std::string &name, int axis, const Tensor &x) {
        if (axis < 0 && x.ndim() > 0 && axis + x.ndim() == 0 && runtime_coupled_.empty()) runtime_coupled_ = kind + " \"" + name + "\" (axis " + std::to_string(axis) + " of a rank-" + std::to_string(x.ndim()) + " input is dim 0)";
    }
    std::vector<int> uses_;
    std::vector<onnx::ValueInfo> inputs_, outputs_;
    size_t fused_away_ = 0;
    size_t conv_pairs_ = 0;
    std::set<int> view_values_;
    int tune_reps_ = 0;
    size_t tuned_ = 0;
    std::map<std::string, GemmPlan> shape_plans_;
    size_t shape_planned_ = 0;
    std::vector<size_t> shape_planned_steps_;
    size_t stats_blocks_ = 0, staged_dql_ = 0, qout_edges_ = 0, dql_loader_steps_ = 0;
    std::unique_ptr<Tensor> stats_arena_, sync_arena_, arena_;

    // what the ConvIntegerToFloat step's own lambda decides per run: does (scale, bias, residual) take the fused epilogue?
    static bool i8_fused_form(const I8Conv &state, const InputList &in, bool &per_channel) {
        const Tensor *scale = in[4], *bias = in[5], *residual = in[6];
        per_channel = false;
        if (!scale) return false;
        const Tensor &x = require(in, 0), &w = require(in, 1);
        bool fused = scale->dtype() == DType::F32 && x.ndim() == 4 && w.ndim() == 4;
        const int64_t o = fused ? w.size(0) : 0;
        if (fused && scale->len() != 1) {
            const auto &sh = scale->shape();
            per_channel = scale->len() == o && ((sh.size() == 4 && sh[0] == 1 && sh[1] == o) || (sh.size() == 3 && sh[0] == o));
            fused = per_channel;
        }
        if (fused && bias) fused = bias->dtype() == DType::F32 && bias->len() == o && bias->ndim() == 4 && bias->size(1) == o;
        if (fused && residual) {
            const rten_hip_conv2d_desc d = state.op->conv.geometry(x.shape(), w.shape());
            fused = residual->dtype() == DType::F32 && residual->shape() == std::vector<int64_t>{d.n, d.o, d.out_h, d.out_w};
        }
        return fused;
    }

    // ---- what the step-level passes below ask of steps_
    bool is_graph_output(int id) const {
        for (auto &o : outputs_) if (ids_.at(o.name) == id) return true;
        return false;
    }
    void index_steps(std::map<int, size_t> &producer, std::map<int, std::vector<size_t>> &consumers) const {
        for (size_t i = 0; i < steps_.size(); i++) {
            for (int id : steps_[i].out) if (id >= 0) producer[id] = i;
            for (int id : steps_[i].in) if (id >= 0) consumers[id].push_back(i);
        }
    }
    void erase_removed_steps() { steps_.erase(std::remove_if(steps_.begin(), steps_.end(), [](const Step &st) { return st.removed; }), steps_.end()); }

    // The staged int8 pipeline at graph level.  A DynamicQuantizeLinear whose codes feed only int8
    // convolutions of one padding geometry writes them straight into the kernel's staged layout; if its input is the f32
    // output of a fused ConvIntegerToFloat step or of a MaxPool, that launch accumulates the min/max the quantizer needs
    // (one statistics block per such tensor, all reset by one launch at the start of a run).
    void plan_int8_staging() {
        std::map<int, size_t> producer;
        std::map<int, std::vector<size_t>> consumers;
        index_steps(producer, consumers);
        struct Pending { size_t dql; size_t producer; };
        std::vector<Pending> want_stats;
        for (size_t i = 0; i < steps_.size(); i++) {
            Step &dq = steps_[i];
            if (dq.kind_name != "DynamicQuantizeLinear" || dq.out.size() < 3 || dq.out[0] < 0 || dq.i8) continue;
            const auto &users = consumers[dq.out[0]];
            if (is_graph_output(dq.out[0]) || users.empty()) continue;
            bool ok = true;
            const Step *first = nullptr;
            for (size_t u : users) {
                const Step &cs = steps_[u];
                if (!cs.i8 || cs.in[0] != dq.out[0] || cs.in[2] != dq.out[2] || !consts_.count(cs.in[1]) || cs.i8->op->conv.padding.same ||
                    cs.i8->op->conv.groups != 1) { ok = false; break; }
                if (std::count(cs.in.begin(), cs.in.end(), dq.out[0]) != 1) { ok = false; break; }
                if (!first) first = &cs;
                else if (cs.i8->op->conv.padding.fixed != first->i8->op->conv.padding.fixed || cs.i8->op->pad_mode != first->i8->op->pad_mode) { ok = false; break; }
            }
            if (!ok || !first) continue;
            auto op = std::make_shared<DynamicQuantizeLinearStaged>();
            op->consumer = *first->i8->op;
            op->kernel = consts_.at(first->in[1]).shape();
            for (size_t u : users) steps_[u].i8->sg.x_staged = true;
            dq.kind_name = "DynamicQuantizeLinear(staged)";
            run_plainly(dq, op);
            dq.dql_staged = op;
            staged_dql_++;
            // fold the following Mul(y_scale, constant scalar) nodes -- one per convolution that reads the codes -- into the quantizer (same f32
            // multiply each): their products become outputs 4, 5, ...
            for (size_t u : consumers[dq.out[1]]) {
                if (op->mul_by.size() >= DynamicQuantizeLinearStaged::kMaxProducts) break;
                Step &mu = steps_[u];
                if (mu.kind_name != "Mul" || mu.in.size() != 2 || mu.removed) continue;
                const int other = mu.in[0] == dq.out[1] ? mu.in[1] : mu.in[0];
                if (other == dq.out[1] || !consts_.count(other) || consts_.at(other).len() != 1 || consts_.at(other).dtype() != DType::F32) continue;
                if (is_graph_output(mu.out[0])) continue;
                op->mul_by.push_back(&consts_.at(other));
                dq.out.push_back(mu.out[0]);
                mu.removed = true;
                fused_away_++;
            }
            auto p = producer.find(dq.in[0]);
            if (p != producer.end() && steps_[p->second].out[0] == dq.in[0] &&
                ((steps_[p->second].i8 && steps_[p->second].i8->to_float) || steps_[p->second].maxpool))
                want_stats.push_back({i, p->second});
        }
        // (indices into steps_ stay valid until here; drop the absorbed Mul steps last)
        struct Eraser { Graph &g; ~Eraser() { g.erase_removed_steps(); } } eraser{*this};
        if (want_stats.empty()) return;
        const size_t sb = rten_hip_minmax_stats_bytes();
        std::map<size_t, size_t> block_of; // producer step -> block
        for (auto &w : want_stats) if (!block_of.count(w.producer)) { const size_t b = block_of.size(); block_of[w.producer] = b; }
        stats_blocks_ = block_of.size();
        stats_arena_.reset(new Tensor(ctx_, {(int64_t)(sb * stats_blocks_)}, DType::U8));
        for (auto &w : want_stats) {
            void *blk = (char *)stats_arena_->ptr() + sb * block_of[w.producer];
            if (steps_[w.producer].maxpool) steps_[w.producer].maxpool->stats_out = blk;
            else steps_[w.producer].i8->sg.stats_out = blk;
            steps_[w.dql].dql_staged->stats_in = blk;
            steps_[w.dql].kind_name = "DynamicQuantizeLinear(staged, producer statistics)";
        }
        if (opt_.qout.empty() && opt_.qout_recompute.empty()) return;
        // Opt-in edges: the quantizer moves INTO its producer's launch.  The merged step produces the conv's f32 tensor (only if somebody else reads
        // it: a residual Add) and the quantizer's outputs; the quantizer's step disappears.  A launch that is refused at run time (its grid is not
        // resident at once) runs the two operators instead, from then on.
        std::vector<Pending> edges;
        for (auto &w : want_stats) {
            Step &P = steps_[w.producer], &D = steps_[w.dql];
            if (!P.i8 || !P.i8->to_float || !(opt_.qout.count(P.name) || opt_.qout_recompute.count(P.name)) || !P.i8->sg.x_staged || !P.i8->sg.packed_weight) continue;
            size_t quantizers = 0;
            for (size_t u : consumers[D.in[0]]) if (steps_[u].dql_staged) quantizers++;
            if (quantizers != 1) continue;
            edges.push_back(w);
        }
        if (edges.empty()) return;
        const size_t gb = rten_hip_grid_sync_bytes();
        sync_arena_.reset(new Tensor(ctx_, {(int64_t)(gb * edges.size())}, DType::U8));
        ctx_.check(rten_hip_grid_sync_reset(ctx_.raw(), sync_arena_->ptr(), (int32_t)edges.size()));
        for (size_t e = 0; e < edges.size(); e++) {
            Step &P = steps_[edges[e].producer], &D = steps_[edges[e].dql];
            const bool keep = consumers[D.in[0]].size() > 1 || is_graph_output(D.in[0]);
            const bool recompute = !opt_.qout.count(P.name); // (listed under "qout2" only: no exchange block is used)
            void *sync = recompute ? nullptr : (char *)sync_arena_->ptr() + gb * e;
            auto state = P.i8;
            state->qout_producer = true;
            auto dql = D.dql_staged;
            auto two_launches = P.run;
            P.run = [state, dql, two_launches, sync, keep, recompute](Context &c, const InputList &in) {
                OutputList out;
                bool per_channel = false;
                if (!state->qout_off && i8_fused_form(*state, in, per_channel)) {
                    if (dql->run_in_producer(c, *state->op, InputList(in.begin(), in.begin() + 4), *in[4], in[5], in[6], state->relu, state->sg, per_channel, sync, keep, out, recompute))
                        return out;
                    state->qout_off = true;
                }
                out = two_launches(c, in);
                OutputList q = dql->run(c, {&out[0]});
                for (Tensor &t : q) out.push_back(std::move(t));
                return out;
            };
            P.out.insert(P.out.end(), D.out.begin(), D.out.end());
            P.kind_name += recompute ? " + DynamicQuantizeLinear(staged) by recomputation (statistics pass + code pass)" : " + DynamicQuantizeLinear(staged) in one launch";
            D.removed = true;
            fused_away_++;
            qout_edges_++;
        }
    }
    // Opt-in per layer (Options::pairs): the f32 Conv step `A` (with whatever Add / Relu it absorbed) and the one f32 Conv step `B` whose input is A's output
    // become ONE step with two outputs, at A's place.  B must take A's output as its data input, constant weights, no residual; the kernel's forms (unit-stride
    // pointwise, K1 = 64, M1 <= 256, M2 in {64, 128}: rten_hip_conv2d_f32_pair_supported) are run-time facts, checked per run -- a pair outside them runs A's and
    // B's own steps one after the other, as the graph spells them.  A's output stays a value of its own: other steps (the next block's residual Add, a downsample
    // layer) still read it.
    void plan_conv_pairs() {
        if (opt_.pairs.empty()) return;
        auto packed_lookup = [&](const std::string &name) -> const Tensor * {
            const auto &tbl = donor_ ? donor_->packed_of_ : packed_of_;
            auto it = tbl.find(name);
            return it == tbl.end() ? nullptr : it->second;
        };
        for (size_t i = 0; i < steps_.size(); i++) {
            Step &A = steps_[i];
            if (!A.conv || A.removed || !opt_.pairs.count(A.name) || A.out.empty() || A.out[0] < 0 || A.in.size() < 4) continue;
            if (A.conv->act.kind != RTEN_HIP_ACT_NONE) continue; // the pair kernel's epilogues know Relu only
            // B: a Conv step reading A's output (constant weights, no residual).  A stage's last block has two such readers -- the next stage's reduce layer and its
            // strided shortcut layer: the one whose attributes fit the kernel (1x1, unit stride, no padding, one group) is taken, whichever comes first in the graph
            auto unit_pointwise = [&](const Step &c) {
                const Tensor &w = consts_.at(c.in[1]);
                const Conv &op = *c.conv;
                return w.ndim() == 4 && w.size(2) == 1 && w.size(3) == 1 && op.groups == 1 && op.strides == std::vector<int>{1, 1} &&
                       (op.padding.same || op.padding.fixed == std::vector<int>{0, 0, 0, 0});
            };
            Step *Bp = nullptr;
            for (size_t k = i + 1; k < steps_.size(); k++) {
                Step &c = steps_[k];
                if (c.conv && !c.removed && c.in.size() >= 4 && c.in[0] == A.out[0] && c.in[3] < 0 && c.in[1] >= 0 && consts_.count(c.in[1]) && (c.in[2] < 0 || consts_.count(c.in[2])) &&
                    c.conv->act.kind == RTEN_HIP_ACT_NONE) {
                    if (!Bp) Bp = &c;
                    if (unit_pointwise(c)) { Bp = &c; break; }
                }
            }
            if (!Bp) continue;
            Step &B = *Bp;
            const Tensor *pa = packed_lookup(A.name), *pb = packed_lookup(B.name);
            if (!pa || !pb) continue;
            const std::shared_ptr<Conv> opa = A.conv, opb = B.conv;
            const auto run_a = A.run, run_b = B.run;
            // the shortcut form: A's residual is the output of a Conv step D (constant weights, no residual, no Relu) that only A reads
            Step *Dp = nullptr;
            const Tensor *pd = nullptr;
            if (opt_.pair_shortcuts.count(A.name) && A.in[3] >= 0) {
                size_t readers = is_graph_output(A.in[3]) ? 2 : 0; // (a graph output is never the one reader's alone)
                for (auto &st : steps_) if (!st.removed) for (int id : st.in) if (id == A.in[3]) readers++;
                for (size_t k = 0; k < i && readers == 1; k++) {
                    Step &c = steps_[k];
                    if (c.conv && !c.removed && !c.out.empty() && c.out[0] == A.in[3] && c.in.size() >= 4 && c.in[3] < 0 && !c.conv->fuse_relu && c.conv->act.kind == RTEN_HIP_ACT_NONE && c.in[1] >= 0 && consts_.count(c.in[1]) &&
                        (c.in[2] < 0 || consts_.count(c.in[2])) && (pd = packed_lookup(c.name)) != nullptr) { Dp = &c; break; }
                }
            }
            const std::shared_ptr<Conv> opd = Dp ? Dp->conv : nullptr;
            const auto run_d = Dp ? Dp->run : run_a;
            if (Dp) A.in[3] = Dp->in[0]; // the step now reads the shortcut's INPUT where it read the shortcut's output
            A.in.push_back(B.in[1]);
            A.in.push_back(B.in[2]);
            if (Dp) { A.in.push_back(Dp->in[1]); A.in.push_back(Dp->in[2]); }
            A.out.push_back(B.out[0]);
            A.kind_name += ">" + B.kind_name;
            A.conv.reset(); // (not a tunable step any more: the one-launch form has no launch plan)
            A.run = [opa, opb, opd, pa, pb, pd, run_a, run_b, run_d](Context &c, const InputList &in) -> OutputList {
                const Tensor &x = require(in, 0), &w1 = require(in, 1), &w2 = require(in, 4);
                const Tensor *b1 = get(in, 2), *res = get(in, 3), *b2 = get(in, 5);
                if (opd) { // shortcut form: in[3] is the shortcut's input, in[6] / in[7] its weights / bias
                    const Tensor &xd = require(in, 3), &wd = require(in, 6);
                    const Tensor *bd = get(in, 7);
                    bool ok = x.dtype() == DType::F32 && xd.dtype() == DType::F32 && x.ndim() == 4 && xd.ndim() == 4 && w1.ndim() == 4 && w2.ndim() == 4 && wd.ndim() == 4 &&
                              opa->groups == 1 && opb->groups == 1 && opd->groups == 1;
                    rten_hip_conv2d_desc d1{}, d2{}, dd{};
                    if (ok) {
                        d1 = opa->geometry(x.shape(), w1.shape());
                        d2 = opb->geometry({d1.n, d1.o, d1.out_h, d1.out_w}, w2.shape());
                        dd = opd->geometry(xd.shape(), wd.shape());
                        ok = rten_hip_conv2d_f32_pair_shortcut_supported(&d1, &dd, &d2) == 1 && (!b1 || (b1->dtype() == DType::F32 && b1->len() == d1.o)) &&
                             (!b2 || (b2->dtype() == DType::F32 && b2->len() == d2.o)) && (!bd || (bd->dtype() == DType::F32 && bd->len() == dd.o));
                    }
                    if (!ok) { // the three steps as they were
                        OutputList r = run_d(c, {in[3], in[6], in[7], nullptr});
                        OutputList y1 = run_a(c, {in[0], in[1], in[2], &r[0]});
                        OutputList y2 = run_b(c, {&y1[0], in[4], in[5], nullptr});
                        y1.push_back(std::move(y2[0]));
                        return y1;
                    }
                    OutputList out;
                    out.emplace_back(c, std::vector<int64_t>{d1.n, d1.o, d1.out_h, d1.out_w}, DType::F32);
                    out.emplace_back(c, std::vector<int64_t>{d2.n, d2.o, d2.out_h, d2.out_w}, DType::F32);
                    c.check(rten_hip_conv2d_f32_pair_shortcut(c.raw(), &d1, (const float *)x.ptr(), (const float *)pa->ptr(), (const float *)vp(b1), &dd, (const float *)xd.ptr(),
                                                              (const float *)pd->ptr(), (const float *)vp(bd), opa->fuse_relu ? RTEN_HIP_CONV_RELU : 0u, (float *)out[0].ptr(), &d2,
                                                              (const float *)pb->ptr(), (const float *)vp(b2), opb->fuse_relu ? RTEN_HIP_CONV_RELU : 0u, (float *)out[1].ptr()));
                    return out;
                }
                bool ok = x.dtype() == DType::F32 && x.ndim() == 4 && w1.ndim() == 4 && w2.ndim() == 4 && w1.dtype() == DType::F32 && w2.dtype() == DType::F32 && opa->groups == 1 && opb->groups == 1;
                rten_hip_conv2d_desc d1{}, d2{};
                if (ok) {
                    d1 = opa->geometry(x.shape(), w1.shape());
                    d2 = opb->geometry({d1.n, d1.o, d1.out_h, d1.out_w}, w2.shape());
                    ok = rten_hip_conv2d_f32_pair_supported(&d1, &d2) == 1 && (!res || (res->dtype() == DType::F32 && res->shape() == std::vector<int64_t>{d1.n, d1.o, d1.out_h, d1.out_w})) &&
                         (!b1 || (b1->dtype() == DType::F32 && b1->len() == d1.o)) && (!b2 || (b2->dtype() == DType::F32 && b2->len() == d2.o));
                }
                if (!ok) { // the two steps as they were
                    OutputList y1 = run_a(c, {in[0], in[1], in[2], in[3]});
                    OutputList y2 = run_b(c, {&y1[0], in[4], in[5], nullptr});
                    y1.push_back(std::move(y2[0]));
                    return y1;
                }
                OutputList out;
                out.emplace_back(c, std::vector<int64_t>{d1.n, d1.o, d1.out_h, d1.out_w}, DType::F32);
                out.emplace_back(c, std::vector<int64_t>{d2.n, d2.o, d2.out_h, d2.out_w}, DType::F32);
                const uint32_t f1 = (opa->fuse_relu ? RTEN_HIP_CONV_RELU : 0u) | (res ? RTEN_HIP_CONV_RESIDUAL : 0u), f2 = opb->fuse_relu ? RTEN_HIP_CONV_RELU : 0u;
                c.check(rten_hip_conv2d_f32_pair(c.raw(), &d1, (const float *)x.ptr(), (const float *)pa->ptr(), (const float *)vp(b1), (const float *)vp(res), f1, (float *)out[0].ptr(),
                                                 &d2, (const float *)pb->ptr(), (const float *)vp(b2), f2, (float *)out[1].ptr()));
                return out;
            };
            B.removed = true;
            fused_away_++;
            conv_pairs_++;
            if (Dp) { Dp->removed = true; fused_away_++; conv_pairs_++; A.kind_name = Dp->kind_name + "+" + A.kind_name; }
        }
        erase_removed_steps();
    }
    // Opt-in per layer (Options::fused_dql, the runner's `fused_layers`): a pointwise ConvIntegerToFloat step whose input comes from a staged
    // quantizer with producer statistics reads the quantizer's f32 INPUT and quantizes in its own operand loader (rten_hip_conv2d_int8_dql:
    // DynamicQuantizeLinear + ConvIntegerToFloat of the reference, src/ops/quantize.rs:352-436 + src/ops/conv.rs:495-587, in one launch, same bits).
    // The quantizer's step stays when another convolution still reads its codes (a stage's shortcut) and goes when none does.
    void plan_dql_loaders() {
        if (opt_.fused_dql.empty()) return;
        std::map<int, size_t> producer;
        std::map<int, std::vector<size_t>> consumers;
        index_steps(producer, consumers);
        for (size_t i = 0; i < steps_.size(); i++) {
            Step &cs = steps_[i];
            if (!cs.i8 || !cs.i8->to_float || cs.i8->qout_producer || !opt_.fused_dql.count(cs.name) || !cs.i8->sg.x_staged || !cs.i8->sg.packed_weight || !cs.i8->sg.packed_weight->len()) continue;
            auto pit = producer.find(cs.in[0]);
            if (pit == producer.end()) continue;
            Step &D = steps_[pit->second];
            if (!D.dql_staged || D.removed || !D.dql_staged->stats_in || D.out.empty() || D.out[0] != cs.in[0]) continue; // (a quantizer merged into its producer has no step)
            // The loader form pays only when the quantizer's own launch DISAPPEARS: every reader of its codes must be a listed, convertible layer.
            // A stage's first 1x1 shares its quantizer with the shortcut convolution: converting it alone keeps the staging launch and swaps a
            // 15-22 us convolution for a 44 us one (measured, session r5c) -- the runner's rule too (`_staged_key == geom`: no loader form).
            {
                bool all_listed = true;
                for (auto &other : steps_) {
                    if (&other == &cs || other.removed) continue;
                    for (size_t k = 0; k < other.in.size() && k < 1; k++)
                        if (other.in[k] == D.out[0] && !(other.i8 && opt_.fused_dql.count(other.name))) all_listed = false;
                    for (size_t k = 1; k < other.in.size(); k++)
                        if (other.in[k] == D.out[0]) all_listed = false; // the codes read as anything but a convolution's X
                }
                if (!all_listed) continue;
            }
            // geometry the loader form covers: 1x1, stride 1, no padding, groups 1, C % 64 == 0 -- all load-time facts
            const Tensor &w = consts_.at(cs.in[1]);
            const Conv &cv = cs.i8->op->conv;
            const bool unit = cv.strides == std::vector<int>{1, 1} && cv.dilations == std::vector<int>{1, 1} && !cv.padding.same && cv.padding.fixed == std::vector<int>{0, 0, 0, 0};
            if (w.ndim() != 4 || w.size(2) != 1 || w.size(3) != 1 || !unit || cv.groups != 1 || w.size(1) % 64 != 0 || w.dtype() != DType::I8) continue;
            if (cs.in[3] >= 0) { // a weight zero point: only the constant scalar 0 of symmetric weights
                auto zi = consts_.find(cs.in[3]);
                if (zi == consts_.end() || zi->second.len() != 1 || zi->second.dtype() != DType::I8 || zi->second.to_host<int8_t>()[0] != 0) continue;
            }
            // the conv's scale must be one of the products Mul(x_scale, w_scale) folded into the quantizer: w_scale is that Mul's constant
            const Tensor *w_scale = nullptr;
            for (size_t k = 0; k < D.dql_staged->mul_by.size(); k++) if (D.out.size() > 3 + k && D.out[3 + k] == cs.in[4]) w_scale = D.dql_staged->mul_by[k];
            if (!w_scale) continue;
            const void *stats_in = D.dql_staged->stats_in;
            auto state = cs.i8;
            const int f32_in = D.in[0];
            cs.in[0] = f32_in; cs.in[2] = -1; cs.in[4] = -1;
            cs.kind_name = "DynamicQuantizeLinear+" + cs.kind_name + " (quantize on load)";
            cs.run = [state, w_scale, stats_in](Context &c, const InputList &in) {
                const Tensor &x = want(require(in, 0), DType::F32, "float32"), &w = require(in, 1);
                const Tensor *bias = in[5], *residual = in[6];
                rten_hip_conv2d_int8_desc di{};
                di.conv = state->op->conv.geometry(x.shape(), w.shape());
                di.x_signed = 0; di.w_signed = 1; di.pad_mode = state->op->pad_mode; di.weights_packed = 1;
                if (bias && bias->len() != di.conv.o) throw OpError(OpError::IncompatibleInputShapes, "bias length does not match output channels");
                if (residual && residual->shape() != std::vector<int64_t>{di.conv.n, di.conv.o, di.conv.out_h, di.conv.out_w})
                    throw OpError(OpError::IncompatibleInputShapes, "quantize-on-load convolution: the residual must have the output's shape");
                Tensor y(c, {di.conv.n, di.conv.o, di.conv.out_h, di.conv.out_w}, DType::F32);
                const uint32_t flags = (state->relu ? RTEN_HIP_CONV_RELU : 0u) | (residual ? RTEN_HIP_CONV_RESIDUAL : 0u);
                c.check(rten_hip_conv2d_int8_dql(c.raw(), &di, (const float *)x.ptr(), stats_in, state->sg.packed_weight->ptr(), (const float *)w_scale->ptr(),
                                                 (const float *)vp(bias), (const float *)vp(residual), flags, (float *)y.ptr(), state->sg.stats_out, nullptr, nullptr));
                OutputList out;
                out.push_back(std::move(y));
                return out;
            };
            dql_loader_steps_++;
            // does anybody still read the quantizer's outputs?
            bool read = false;
            for (auto &st : steps_) {
                if (&st == &D || st.removed) continue;
                for (int id : st.in) for (int o : D.out) if (id >= 0 && id == o) read = true;
            }
            for (int oid : D.out) if (is_graph_output(oid)) read = true;
            if (!read) { D.removed = true; fused_away_++; }
        }
        erase_removed_steps();
    }
    uint64_t graph_ = 0;
    std::vector<Tensor> captured_outputs_;

    void tune_step(Step &st, const InputList &in) {
        std::vector<GemmPlan> plans;
        const int nvar = rten_hip_num_gemm_variants();
        auto set_plan = [&](const GemmPlan &p) { if (st.conv) st.conv->plan = p; else *st.gemm_plan = p; };
        if (st.gemm_plan) {
            // MatMul-family steps (row-major A): the LDS-DMA pipelines with three / four stages x tile order (m fastest / n fastest within an XCD's
            // share: which operand stays L2-resident) -- the candidate set of rten_amd/workloads/bert.py::autotune
            for (int v : {0, 1, 2, 3, 12, 13, 14, 15}) if (v < nvar) for (int o = 0; o < 2; o++) plans.push_back(GemmPlan{true, v, 3, 1, o});
            // + the small-M weight-streaming kernel (variant 31: one batch, M <= 64; any other call runs it as variant 3, i.e. a duplicate candidate)
            if (31 < nvar) plans.push_back(GemmPlan{true, 31, 3, 1, 0});
        } else {
        const Tensor &w = require(in, 1);
        const int64_t k = w.len() / std::max<int64_t>(w.size(0), 1); // per-group depth C/g * kh * kw
        const int nblk = (int)((k + 255) / 256);
        for (int v = 0; v < nvar; v++) for (int o = 0; o < 2; o++) plans.push_back(GemmPlan{true, v, 0, 1, o});
        // thin-tile tail (split mode 4) on the LDS-DMA pipelines: whole rounds with the variant's tile + 16x64 tiles on 16x16x4 MFMAs
        for (int v = 0; v < nvar; v++) if (v < 4 || v >= 12) for (int o = 0; o < 2; o++) plans.push_back(GemmPlan{true, v, 4, 1, o});
        // persistent plan (split mode 5, groups = workgroups per compute unit): tile list per workgroup, DMA across tile boundaries
        for (int v : {0, 1, 2, 3, 20, 21, 22, 23}) if (v < nvar) for (int r = 1; r <= 4; r++) for (int o = 0; o < 2; o++) plans.push_back(GemmPlan{true, v, 5, r, o});
        // lean persistent kernel (split mode 6: 64x64 tiles, K a multiple of 32)
        for (int r = 1; r <= 3; r++) for (int o = 0; o < 2; o++) plans.push_back(GemmPlan{true, 3, 6, r, o});
        if (nblk > 1) {
            static const int split_variants[] = {0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15, 16, 17, 18, 19};
            for (int v : split_variants) {
                if (v >= nvar) continue;
                std::set<int> group_counts;
                for (int g : {2, 3, 4, 6, nblk}) if (g >= 2 && g <= nblk) group_counts.insert(g);
                for (int g : group_counts) {
                    plans.push_back(GemmPlan{true, v, 1, g, 0});
                    for (int o : {0, 2, 3}) plans.push_back(GemmPlan{true, v, 2, g, o});
                }
            }
        }
        }
        GemmPlan best;
        float best_ms = 1e30f;
        for (const GemmPlan &p : plans) {
            set_plan(p);
            try {
                st.run(ctx_, in); // warm (also grows the split-K slab scratch before any capture)
                float ms = 1e30f;
                for (int round = 0; round < 2; round++) { // best of two short runs
                    ctx_.check(rten_hip_timer_start(ctx_.raw(), 2));
                    for (int r = 0; r < tune_reps_; r++) st.run(ctx_, in);
                    ctx_.check(rten_hip_timer_stop(ctx_.raw(), 2));
                    float t = 0;
                    ctx_.check(rten_hip_timer_elapsed_ms(ctx_.raw(), 2, &t));
                    ms = std::min(ms, t / (float)tune_reps_);
                }
                if (ms < best_ms) { best_ms = ms; best = p; }
            } catch (const OpError &) { // a plan the kernel family does not offer for this shape
            }
        }
        set_plan(best);
        tuned_++;
    }

    int id_of(const std::string &n) {
        if (n.empty()) return -1; // omitted optional input
        auto it = ids_.find(n);
        if (it != ids_.end()) return it->second;
        const int id = (int)names_.size();
        names_.push_back(n);
        ids_[n] = id;
        return id;
    }

    static DType dtype_of(int onnx_type, const std::string &what) {
        switch (onnx_type) {
        case onnx::FLOAT: return DType::F32;
        case onnx::INT32: case onnx::INT64: case onnx::BOOL: return DType::I32; // int64 and bool are int32 from load on (onnx_loader.rs:332-339,464-492)
        case onnx::UINT8: return DType::U8;
        case onnx::INT8: return DType::I8;
        default: throw GraphError("unsupported tensor element type " + std::to_string(onnx_type) + " (" + what + ")");
        }
    }

    Tensor upload(const onnx::TensorProto &t) {
        const DType dt = dtype_of(t.data_type, t.name);
        const int64_t n = t.len();
        const size_t esz = t.data_type == onnx::INT64 ? 8 : t.data_type == onnx::BOOL ? 1 : dtype_size(dt);
        if ((size_t)n * esz != t.raw.size()) throw GraphError("initializer " + t.name + ": data size does not match its dims");
        // small integer / float constants keep a host copy: the operands of shape arithmetic (hostops above)
        constexpr int64_t kHostConst = 4096;
        if (t.data_type == onnx::INT64 || t.data_type == onnx::BOOL) {
            std::vector<int32_t> narrow((size_t)n);
            for (int64_t i = 0; i < n; i++) {
                if (t.data_type == onnx::BOOL) { narrow[(size_t)i] = t.raw[(size_t)i] != 0; continue; }
                int64_t v;
                std::memcpy(&v, t.raw.data() + 8 * i, 8);
                narrow[(size_t)i] = (int32_t)std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v)); // saturating, like the loader
            }
            Tensor d = Tensor::from_host<int32_t>(ctx_, t.dims, narrow.data());
            if (n <= kHostConst) { auto h = std::make_shared<HostVal>(); h->shape = t.dims; h->i.assign(narrow.begin(), narrow.end()); d.set_host(h); }
            return d;
        }
        Tensor d(ctx_, t.dims, dt);
        if (d.bytes() && !(opt_.skip_large_uploads && d.bytes() >= ((size_t)64 << 10)))
            ctx_.check(rten_hip_memcpy_h2d(ctx_.raw(), d.ptr(), t.raw.data(), d.bytes()));
        if (n <= kHostConst && (dt == DType::I32 || dt == DType::F32)) {
            auto h = std::make_shared<HostVal>();
            h->shape = t.dims;
            h->is_float = dt == DType::F32;
            if (h->is_float) { h->f.resize((size_t)n); std::memcpy(h->f.data(), t.raw.data(), (size_t)n * 4); }
            else { h->i.resize((size_t)n); for (int64_t i = 0; i < n; i++) { int32_t v; std::memcpy(&v, t.raw.data() + 4 * i, 4); h->i[(size_t)i] = v; } }
            d.set_host(h);
        }
        return d;
    }

    // ---- host-evaluated steps (hostops above).  The device copy of a host-computed value is made once per distinct value and cached with the step, the
    // latest 8 values each.  Input shapes may change from one run to the next (one Graph serves every binding of its dynamic axes); they are fixed WITHIN
    // capture(): its eager warm-up run fills the cache and the captured run only finds hits (an upload inside a capture would be recorded with the host
    // pointer: refused).  The captured graph reads the copies at their addresses, so one that existed when a capture was made is parked, not released, when
    // later eager runs at other shapes push it out of the cache (Context::retire states the bound).  What a step returns is a view of the cached copy:
    // good for the run that asked; run() hands a graph output out as a copy of it.
    struct HostCache {
        struct Entry { std::shared_ptr<const HostVal> host; std::unique_ptr<Tensor> copy; uint64_t born; };
        std::vector<Entry> entries;
    };
    static Tensor materialize(Context &c, HostVal &&hv, HostCache &cache) {
        for (auto &e : cache.entries)
            if (*e.host == hv) { Tensor v = Tensor::view_of(*e.copy, e.copy->shape()); v.set_host(e.host); return v; }
        if (rten_hip_capture_active(c.raw()))
            throw GraphError("a shape-dependent constant changed between the warm-up run and the capture (input shapes must stay fixed while a graph is captured)");
        auto h = std::make_shared<const HostVal>(std::move(hv));
        std::unique_ptr<Tensor> t;
        // (not from the pool: the cached copy stays, and a pool buffer taken here -- say the 8 bytes of a [2] shape vector, which are also the 8 bytes of a
        //  [2, 1] activation -- would be missing in the captured run that follows, whose first request of that size would then allocate inside the capture)
        if (h->is_float) t.reset(new Tensor(Tensor::from_host_unpooled<float>(c, h->shape, h->f.data())));
        else { std::vector<int32_t> w(h->i.begin(), h->i.end()); t.reset(new Tensor(Tensor::from_host_unpooled<int32_t>(c, h->shape, w.data()))); }
        if (cache.entries.size() >= 8) { // (shapes changed a few times: keep the recent ones)
            cache.entries.front().copy->retire(cache.entries.front().born);
            cache.entries.erase(cache.entries.begin());
        }
        cache.entries.push_back({h, std::move(t), c.stamp()});
        Tensor v = Tensor::view_of(*cache.entries.back().copy, h->shape);
        v.set_host(h);
        return v;
    }
    static std::vector<int64_t> host_ints(const Tensor *t, const std::string &what) {
        if (!t) return {};
        if (!t->host() || t->host()->is_float) throw OpError(OpError::UnsupportedValue, what + " must be a constant or computable from the input shapes (it depends on device data)");
        return t->host()->i;
    }
    // A step that runs on the host when every operand carries a host value (`hf` returns false to decline) and on the device otherwise.
    using HostFn = std::function<bool(const std::vector<const HostVal *> &, HostVal &)>;
    using DevFn = std::function<OutputList(Context &, const InputList &)>;
    static void make_hostable(Step &st, HostFn hf, DevFn df) {
        auto cache = std::make_shared<HostCache>();
        st.run = [hf, df, cache](Context &c, const InputList &in) {
            bool all = true;
            std::vector<const HostVal *> hv;
            for (const Tensor *t : in) {
                if (!t) { hv.push_back(nullptr); continue; }
                if (!t->host()) { all = false; break; }
                hv.push_back(t->host());
            }
            if (all) {
                HostVal out;
                if (hf(hv, out)) {
                    OutputList o;
                    o.push_back(materialize(c, std::move(out), *cache));
                    return o;
                }
            }
            return df(c, in);
        };
    }

    // `spatial`: the number of spatial axes the node's attributes are written for (2, or 1 for a 1-D convolution)
    static Padding padding_of(const onnx::Node &n, const char *op, size_t spatial = 2) {
        const onnx::Attr *ap = n.attr("auto_pad");
        if (ap && !ap->s.empty() && ap->s != "NOTSET") {
            if (ap->s == "SAME_UPPER") return Padding::Same();
            if (ap->s == "VALID") return Padding::Fixed(std::vector<int>(2 * spatial, 0));
            throw GraphError(std::string(op) + " " + n.name + ": auto_pad " + ap->s + " is not supported");
        }
        std::vector<int> p = n.get_ints("pads", std::vector<int>(2 * spatial, 0));
        if (p.size() != 2 * spatial)
            throw GraphError(std::string(op) + " " + n.name + (spatial == 1 ? ": a 1-D operator takes 2 pad values" : ": only 2-D spatial operators are supported"));
        return Padding::Fixed(p); // ONNX [top, left, bottom, right] == the reference's order; 1-D: [begin, end]
    }
    // A 1-D Conv node keeps one-axis attributes, defaults included: the operator expands a [N, C, W] input to 2-D itself (src/ops/conv.rs:142-182) and
    // asks for exactly these lengths.  `weight_rank`: the rank of a constant weight (3 decides for 1-D, 4 for 2-D); 0, a run-time weight: an
    // attribute of one-axis length (kernel_shape / strides / dilations of one value, pads of two) decides.
    static Conv conv_attrs(const onnx::Node &n, int weight_rank = 0) {
        Conv c;
        const bool hinted = n.get_ints("kernel_shape", {}).size() == 1 || n.get_ints("strides", {}).size() == 1 || n.get_ints("dilations", {}).size() == 1 ||
                            n.get_ints("pads", {}).size() == 2;
        const bool one_d = weight_rank ? weight_rank == 3 : hinted;
        const std::vector<int> ones(one_d ? 1 : 2, 1);
        c.groups = (int)n.get_int("group", 1);
        c.dilations = n.get_ints("dilations", ones);
        c.strides = n.get_ints("strides", ones);
        c.padding = padding_of(n, "Conv", one_d ? 1 : 2);
        return c;
    }

    // ---- canonicalisation of exporter idioms, on the ONNX node list (the reference does these in its graph optimiser, so its
    //      numerics are the FUSED operators' numerics -- they are applied whether or not the backend's own epilogue fusions are on):
    //   * Constant nodes become initializers (`Constant` -> constant node, rten-onnx loader);
    //   * x * Sigmoid(x) -> Silu, x * Sigmoid(alpha * x) -> Swish                          (SiluFusion / SwishFusion, fusions.rs:567-615)
    //   * x * (Erf(x / sqrt(2) | x * (1 / sqrt(2))) + 1) * 0.5                              -> Gelu               (GeluFusion, optimize/fusions.rs:407-430)
    //   * (x - ReduceMean(x)) / Sqrt(eps + ReduceMean(Pow(x - ReduceMean(x), 2))) * scale [+ bias], means over the last axis
    //                                                                                      -> LayerNormalization (fusions.rs:674-747)
    //     (PyTorch's exporter writes nn.LayerNorm and nn.GELU this way).
    static onnx::Model canonicalize(const onnx::Model &src) {
        onnx::Model m = src;
        for (auto &n : m.nodes)
            if (n.op_type == "Constant" && n.outputs.size() == 1) {
                const onnx::Attr *v = n.attr("value");
                if (!v) throw GraphError("Constant " + n.name + ": only the tensor `value` form is supported");
                onnx::TensorProto t = v->t;
                t.name = n.outputs[0];
                m.initializers.push_back(std::move(t));
                n.op_type.clear(); // removed below
            }
        { // ---- DequantizeLinear over initializers -> an f32 initializer (fold_dequantize); an int8 / int32 initializer left without a reader is dropped
            std::map<std::string, size_t> init_at;
            for (size_t i = 0; i < m.initializers.size(); i++) init_at[m.initializers[i].name] = i;
            std::set<std::string> graph_outs, folded_operands;
            for (auto &o : m.outputs) graph_outs.insert(o.name);
            for (auto &n : m.nodes) {
                if (n.op_type != "DequantizeLinear" || !(n.domain.empty() || n.domain == "ai.onnx") || n.inputs.size() < 2 || n.outputs.size() != 1 || graph_outs.count(n.outputs[0])) continue;
                const bool has_zp = n.inputs.size() > 2 && !n.inputs[2].empty();
                if (!init_at.count(n.inputs[0]) || !init_at.count(n.inputs[1]) || (has_zp && !init_at.count(n.inputs[2]))) continue;
                onnx::TensorProto y = fold_dequantize(n, m.initializers[init_at[n.inputs[0]]], m.initializers[init_at[n.inputs[1]]], has_zp ? &m.initializers[init_at[n.inputs[2]]] : nullptr);
                for (auto &in : n.inputs) if (!in.empty()) folded_operands.insert(in);
                init_at[y.name] = m.initializers.size();
                m.initializers.push_back(std::move(y));
                m.folded_dequantize++;
                n.op_type.clear();
            }
            if (m.folded_dequantize) {
                for (auto &n : m.nodes) if (!n.op_type.empty()) for (auto &in : n.inputs) folded_operands.erase(in);
                for (auto &o : graph_outs) folded_operands.erase(o);
                std::vector<onnx::TensorProto> kept;
                for (auto &t : m.initializers) if (!folded_operands.count(t.name)) kept.push_back(std::move(t));
                m.initializers = std::move(kept);
            }
        }
        { // (the nodes taken out above go first: the matcher below indexes the list)
            std::vector<onnx::Node> live;
            for (auto &n : m.nodes) if (!n.op_type.empty()) live.push_back(std::move(n));
            m.nodes = std::move(live);
        }
        // ---- Silu / Swish / Gelu / LayerNormalization, matched and applied by the reference's own rules (tests/fusion_rules.py restates them with
        //      their cites and tests/test_fusion_rules.py pins them):
        //   * operator name and operand count; a commutative binary operator in either order; Add / Mul chains of >= 3 pattern operands as a
        //     multiset under any bracketing (pattern_matcher.rs:139-197); one symbol, one value; float constants of one element within ABSOLUTE 1e-4;
        //   * operators visited last to first, the first fusion in list order that matches wins; a fusion whose operators an earlier one of the
        //     round has claimed is skipped; one whose interior values are read elsewhere or are graph outputs is dropped AFTER claiming its operators
        //     for the round; rounds repeat while one applied, three at the most (optimize.rs:119-260, 611-660).
        //   A ReduceMean whose axes are a rank-1 constant input counts as the attribute form from the round after ReduceMeanAxesFusion (fusions.rs:371-404) took it.
        struct Pat {
            enum Kind { Op, Const, Sym, Any } kind = Op;
            std::string name, key;  // Op: operator name and optional key; Sym: the symbol
            std::vector<Pat> in;    // Op: operand patterns; Any: alternatives, tried left to right
            float value = 0.f;      // Const, tolerance 1e-4
            bool constant = false;  // Sym: matches constants only
            static Pat op(const char *name, std::vector<Pat> in, const char *key = "") { Pat p; p.name = name; p.in = std::move(in); p.key = key; return p; }
            static Pat c(float v) { Pat p; p.kind = Const; p.value = v; return p; }
            static Pat sym(const char *name, bool constant = false) { Pat p; p.kind = Sym; p.name = name; p.constant = constant; return p; }
            static Pat any(std::vector<Pat> alts) { Pat p; p.kind = Any; p.in = std::move(alts); return p; }
        };
        typedef std::vector<std::pair<std::string, std::string>> Syms; // symbol or key -> value name (for a key: the output of the operator)
        struct Matcher {
            const onnx::Model &m;
            std::map<std::string, size_t> producer;
            std::map<std::string, std::vector<size_t>> consumers;
            std::map<std::string, const onnx::TensorProto *> inits;
            std::set<std::string> graph_outs;
            const std::set<std::string> &attr_form; // outputs of the ReduceMean nodes whose constant axes input counts as the attribute
            Matcher(const onnx::Model &model, const std::set<std::string> &converted) : m(model), attr_form(converted) {
                for (size_t i = 0; i < m.nodes.size(); i++) {
                    for (auto &o : m.nodes[i].outputs) if (!o.empty()) producer[o] = i;
                    for (auto &in : m.nodes[i].inputs) if (!in.empty()) consumers[in].push_back(i);
                }
                for (auto &t : m.initializers) inits[t.name] = &t;
                for (auto &o : m.outputs) graph_outs.insert(o.name);
            }
            bool is_const(const std::string &v) const { return inits.count(v) != 0; }
            long made_by(const std::string &v) const { auto it = producer.find(v); return is_const(v) || it == producer.end() ? -1 : (long)it->second; }
            bool scalar(const std::string &v, float &out) const { // one element at any rank (TensorView::item)
                auto it = inits.find(v);
                if (it == inits.end() || it->second->data_type != onnx::FLOAT || it->second->len() != 1 || it->second->raw.size() != 4) return false;
                std::memcpy(&out, it->second->raw.data(), 4);
                return true;
            }
            bool axes_of(const onnx::Node &n, std::vector<int64_t> &axes) const { // the attribute, or a rank-1 int64 constant input
                axes.clear();
                if (n.inputs.size() == 2 && !n.inputs[1].empty()) {
                    auto it = inits.find(n.inputs[1]);
                    if (it == inits.end() || it->second->data_type != onnx::INT64 || it->second->dims.size() != 1 || it->second->raw.size() != 8 * (size_t)it->second->len()) return false;
                    axes.resize((size_t)it->second->len());
                    if (!axes.empty()) std::memcpy(axes.data(), it->second->raw.data(), it->second->raw.size());
                    return true;
                }
                const onnx::Attr *a = n.attr("axes");
                if (!a) return false;
                axes = a->ints;
                return true;
            }
            // a ReduceMean that an earlier round has turned into the attribute form (ReduceMeanAxesFusion) has one operand for the patterns
            size_t arity(const onnx::Node &n) const { return n.op_type == "ReduceMean" && n.inputs.size() == 2 && attr_form.count(n.outputs.at(0)) ? 1 : n.inputs.size(); }
            static bool commutative(const std::string &op) { return op == "Add" || op == "Mul" || op == "And" || op == "Or" || op == "Xor" || op == "Equal"; }
            static bool associative(const std::string &op) { return op == "Add" || op == "Mul"; }
            static const std::string *find(const Syms &s, const std::string &name) { for (auto &kv : s) if (kv.first == name) return &kv.second; return nullptr; }
            static void flatten_pattern(const Pat &p, const std::string &name, std::vector<const Pat *> &out) {
                if (p.kind == Pat::Op && p.name == name && p.in.size() == 2 && p.key.empty()) for (auto &q : p.in) flatten_pattern(q, name, out);
                else out.push_back(&p);
            }
            void flatten_graph(const std::string &v, const std::string &name, std::vector<std::string> &out) const {
                const long i = made_by(v);
                if (i >= 0 && m.nodes[(size_t)i].op_type == name && m.nodes[(size_t)i].inputs.size() == 2 && !m.nodes[(size_t)i].inputs[0].empty() && !m.nodes[(size_t)i].inputs[1].empty())
                    for (auto &s : m.nodes[(size_t)i].inputs) flatten_graph(s, name, out);
                else out.push_back(v);
            }
            bool match_set(const std::vector<const Pat *> &pats, size_t at, const std::vector<std::string> &vals, std::vector<bool> &used, Syms &syms) const {
                if (at == pats.size()) return true;
                for (size_t i = 0; i < vals.size(); i++) {
                    if (used[i]) continue;
                    const size_t mark = syms.size();
                    if (test(*pats[at], vals[i], syms)) {
                        used[i] = true;
                        if (match_set(pats, at + 1, vals, used, syms)) return true;
                        used[i] = false;
                    }
                    syms.resize(mark);
                }
                return false;
            }
            bool match_op(const Pat &p, size_t idx, Syms &syms) const {
                const onnx::Node &n = m.nodes[idx];
                if (!(n.domain.empty() || n.domain == "ai.onnx") || n.op_type != p.name || p.in.size() != arity(n)) return false;
                const bool both = p.in.size() == 2 && !n.inputs[0].empty() && !n.inputs[1].empty();
                if (associative(p.name) && commutative(p.name) && p.in.size() == 2) {
                    std::vector<const Pat *> pats;
                    for (auto &q : p.in) flatten_pattern(q, p.name, pats);
                    if (pats.size() >= 3) {
                        std::vector<std::string> vals;
                        if (both) for (auto &s : n.inputs) flatten_graph(s, p.name, vals);
                        std::vector<bool> used(vals.size(), false);
                        if (pats.size() == vals.size() && match_set(pats, 0, vals, used, syms)) return true;
                    }
                }
                if (commutative(p.name) && both) {
                    const size_t mark = syms.size();
                    if (test(p.in[0], n.inputs[0], syms) && test(p.in[1], n.inputs[1], syms)) return true;
                    syms.resize(mark);
                    return test(p.in[1], n.inputs[0], syms) && test(p.in[0], n.inputs[1], syms);
                }
                for (size_t k = 0; k < p.in.size(); k++) if (n.inputs[k].empty() || !test(p.in[k], n.inputs[k], syms)) return false;
                return true;
            }
            bool test(const Pat &p, const std::string &v, Syms &syms) const { // pattern against a value
                if (p.kind == Pat::Any) {
                    for (auto &q : p.in) {
                        const size_t mark = syms.size();
                        if (test(q, v, syms)) return true;
                        syms.resize(mark);
                    }
                    return false;
                }
                if (p.kind == Pat::Op) {
                    const long i = made_by(v);
                    if (i < 0 || !match_op(p, (size_t)i, syms)) return false;
                    if (!p.key.empty()) syms.emplace_back(p.key, v);
                    return true;
                }
                if (p.kind == Pat::Const) { float c; return scalar(v, c) && std::fabs(c - p.value) <= 1e-4f; }
                if (p.constant && !is_const(v)) return false;
                if (const std::string *seen = find(syms, p.name)) return *seen == v;
                syms.emplace_back(p.name, v);
                return true;
            }
            bool match_root(const Pat &p, size_t idx, Syms &syms) const { // pattern against an operator
                syms.clear();
                if (p.kind == Pat::Any) {
                    for (auto &q : p.in) { if (match_root(q, idx, syms)) return true; }
                    return false;
                }
                return p.kind == Pat::Op && match_op(p, idx, syms);
            }
            // the rank the reference's shape inference gives a value, as far as the idioms need it: declared for a graph input, carried through broadcasting
            // binary operators, Sqrt and ReduceMean (binary_elementwise.rs:534,697,949,1120,1184; reduce.rs:579); -1: unknown
            long rank_of(const std::string &v, int depth = 0) const {
                if (v.empty() || depth > 16) return -1;
                auto it = inits.find(v);
                if (it != inits.end()) return (long)it->second->dims.size();
                for (auto &in : m.inputs) if (in.name == v) return in.dims.empty() ? -1 : (long)in.dims.size();
                const long i = made_by(v);
                if (i < 0) return -1;
                const onnx::Node &n = m.nodes[(size_t)i];
                if ((n.op_type == "Add" || n.op_type == "Sub" || n.op_type == "Mul" || n.op_type == "Div" || n.op_type == "Pow") && n.inputs.size() == 2) {
                    const long a = rank_of(n.inputs[0], depth + 1), b = rank_of(n.inputs[1], depth + 1);
                    return a < 0 || b < 0 ? -1 : std::max(a, b);
                }
                if (n.op_type == "Sqrt" && n.inputs.size() == 1) return rank_of(n.inputs[0], depth + 1);
                if (n.op_type == "ReduceMean" && !n.inputs.empty()) {
                    const long r = rank_of(n.inputs[0], depth + 1);
                    std::vector<int64_t> axes;
                    if (r < 0 || n.get_int("keepdims", 1) == 1) return r;
                    return axes_of(n, axes) ? r - (long)axes.size() : -1;
                }
                return -1;
            }
            bool last_axis_mean(const std::string &mean_out) const { // op_applied_to_last_axis::<ReduceMean> (fusions.rs:643-671)
                const long i = made_by(mean_out);
                std::vector<int64_t> axes;
                if (i < 0 || !axes_of(m.nodes[(size_t)i], axes) || axes.size() != 1) return false;
                if (axes[0] == -1) return true;
                const long r = rank_of(m.nodes[(size_t)i].inputs[0]);
                return r >= 1 && r - 1 == (long)axes[0];
            }
        };
        const float sqrt2 = std::sqrt(2.0f);
        const Pat x = Pat::sym("x");
        const Pat center = Pat::op("Sub", {x, Pat::op("ReduceMean", {x}, "center_mean")});
        const Pat normalized = Pat::op("Div", {center, Pat::op("Sqrt", {Pat::op("Add", {Pat::sym("epsilon", true), Pat::op("ReduceMean", {Pat::op("Pow", {center, Pat::c(2.0f)})}, "norm_mean")})})});
        const Pat scaled = Pat::op("Mul", {normalized, Pat::sym("scale", true)});
        const std::vector<std::pair<std::string, Pat>> fusions = { // in the reference's list order (optimize.rs:622-629)
            {"Silu", Pat::op("Mul", {x, Pat::op("Sigmoid", {x})})},
            {"Swish", Pat::op("Mul", {x, Pat::op("Sigmoid", {Pat::op("Mul", {Pat::sym("alpha", true), x})})})},
            {"Gelu", Pat::op("Mul", {Pat::op("Mul", {x, Pat::op("Add", {Pat::op("Erf", {Pat::any({Pat::op("Div", {x, Pat::c(sqrt2)}), Pat::op("Mul", {x, Pat::c(1.0f / sqrt2)})})}), Pat::c(1.0f)})}), Pat::c(0.5f)})},
            {"LayerNormalization", Pat::any({Pat::op("Add", {scaled, Pat::sym("bias", true)}), scaled})},
        };
        std::set<std::string> attr_form;
        for (int round = 0; round < 3; round++) {
            const Matcher g(m, attr_form);
            std::set<size_t> claimed, gone;
            std::set<std::string> converted; // by this round: seen by the patterns from the next round on, as in the reference
            std::map<size_t, onnx::Node> fused_at;
            for (size_t idx = m.nodes.size(); idx-- > 0;) {
                if (claimed.count(idx)) continue;
                { // ReduceMeanAxesFusion, first in the list: ReduceMean(x, axes constant, a rank-1 integer vector) -> the attribute form.  It spends a round
                  // and claims the node, as every fusion does; the node itself stays as written (the step builder reads either form).
                    const onnx::Node &n = m.nodes[idx];
                    std::vector<int64_t> axes;
                    if ((n.domain.empty() || n.domain == "ai.onnx") && n.op_type == "ReduceMean" && n.inputs.size() == 2 && n.outputs.size() == 1 && !attr_form.count(n.outputs[0]) && g.axes_of(n, axes)) {
                        claimed.insert(idx);
                        converted.insert(n.outputs[0]);
                        continue;
                    }
                }
                for (auto &f : fusions) {
                    Syms syms;
                    if (!g.match_root(f.second, idx, syms)) continue;
                    const onnx::Node &root = m.nodes[idx];
                    onnx::Node fn;
                    fn.op_type = f.first;
                    fn.inputs = {*Matcher::find(syms, "x")};
                    if (f.first == "Swish") {
                        onnx::Attr a;
                        a.name = "alpha"; a.type = 1;
                        if (!g.scalar(*Matcher::find(syms, "alpha"), a.f)) continue; // "alpha not a scalar"
                        fn.attrs = {a};
                    } else if (f.first == "LayerNormalization") {
                        onnx::Attr axis, epsilon;
                        axis.name = "axis"; axis.type = 2; axis.i = -1;
                        epsilon.name = "epsilon"; epsilon.type = 1;
                        if (!g.last_axis_mean(*Matcher::find(syms, "norm_mean")) || !g.last_axis_mean(*Matcher::find(syms, "center_mean")) || !g.scalar(*Matcher::find(syms, "epsilon"), epsilon.f)) continue;
                        fn.attrs = {axis, epsilon};
                        fn.inputs.push_back(*Matcher::find(syms, "scale"));
                        if (const std::string *bias = Matcher::find(syms, "bias")) fn.inputs.push_back(*bias);
                    }
                    std::string lower = f.first == "LayerNormalization" ? "layer_norm" : f.first;
                    lower[0] = (char)std::tolower(lower[0]);
                    fn.name = root.name.empty() ? lower : root.name;
                    fn.outputs = root.outputs;
                    // the operators between the fused node's inputs and the root
                    std::vector<size_t> ops, stack = {idx};
                    while (!stack.empty()) {
                        const size_t i = stack.back();
                        stack.pop_back();
                        if (std::find(ops.begin(), ops.end(), i) != ops.end()) continue;
                        ops.push_back(i);
                        for (auto &s : m.nodes[i].inputs)
                            if (!s.empty() && std::find(fn.inputs.begin(), fn.inputs.end(), s) == fn.inputs.end() && g.made_by(s) >= 0) stack.push_back((size_t)g.made_by(s));
                    }
                    std::sort(ops.begin(), ops.end());
                    bool usable = true;
                    for (size_t o : ops) { // claimed one by one: what was walked before a clash stays claimed
                        if (claimed.count(o)) { usable = false; break; }
                        claimed.insert(o);
                    }
                    for (size_t o : ops)
                        for (auto &v : m.nodes[o].outputs) {
                            if (!usable || v.empty() || std::find(root.outputs.begin(), root.outputs.end(), v) != root.outputs.end()) continue;
                            if (g.graph_outs.count(v)) usable = false;
                            auto us = g.consumers.find(v);
                            if (us != g.consumers.end()) for (size_t c : us->second) if (!std::binary_search(ops.begin(), ops.end(), c)) usable = false;
                        }
                    if (usable) {
                        for (size_t o : ops) if (o != idx) gone.insert(o);
                        fused_at[idx] = std::move(fn);
                    }
                    break; // the first fusion that matched decides this operator, applied or not
                }
            }
            if (fused_at.empty() && converted.empty()) break;
            attr_form.insert(converted.begin(), converted.end());
            std::vector<onnx::Node> next;
            for (size_t i = 0; i < m.nodes.size(); i++) {
                auto it = fused_at.find(i);
                if (it != fused_at.end()) next.push_back(std::move(it->second));
                else if (!gone.count(i)) next.push_back(std::move(m.nodes[i]));
            }
            m.nodes = std::move(next);
        }
        std::vector<onnx::Node> kept;
        for (auto &n : m.nodes) if (!n.op_type.empty()) kept.push_back(std::move(n));
        m.nodes = std::move(kept);
        return m;
    }

    // ---- what the fusion matchers ask of the ONNX node list.  `dead`: nodes an earlier step has taken.  A fused step runs at the position of the LAST node it
    //      absorbs (st.pos), where -- the node list being topologically sorted -- every operand of every absorbed node is already available.
    struct Nodes {
        Graph &g;
        const onnx::Model &m;
        std::map<std::string, std::vector<size_t>> users; // consumers of every value
        std::map<std::string, size_t> producer;
        std::set<std::string> graph_outs; // graph outputs count as a use: they must not be fused away
        std::vector<bool> dead;
        Nodes(Graph &g_, const onnx::Model &m_) : g(g_), m(m_), dead(m_.nodes.size(), false) {
            for (size_t i = 0; i < m.nodes.size(); i++) {
                for (auto &s : m.nodes[i].inputs) if (!s.empty()) users[s].push_back(i);
                for (auto &s : m.nodes[i].outputs) if (!s.empty()) producer[s] = i;
            }
            for (auto &o : m.outputs) graph_outs.insert(o.name);
        }
        const onnx::Node &operator[](long i) const { return m.nodes[(size_t)i]; }
        // the one live node reading v, unless v is a graph output; -1 otherwise
        long sole_reader(const std::string &v) const {
            if (graph_outs.count(v)) return -1;
            auto it = users.find(v);
            if (it == users.end() || it->second.size() != 1 || dead.at(it->second[0])) return -1;
            return (long)it->second[0];
        }
        long sole_user(const std::string &v, const char *op) const { const long u = sole_reader(v); return u >= 0 && m.nodes[(size_t)u].op_type == op ? u : -1; }
        // the sole consumer of v if it is an activation activation_of takes (and not a graph output); -1 otherwise
        long sole_activation(const std::string &v, Activation &a) const {
            const long u = sole_reader(v);
            if (u < 0) return -1;
            const onnx::Node &un = m.nodes[(size_t)u];
            return un.inputs.size() >= 1 && un.inputs[0] == v && g.activation_of(un, a) ? u : -1;
        }
        // the live `op` node producing v, if v has one reader and is not a graph output; -1 otherwise
        long made_by(const std::string &v, const char *op) const {
            auto it = producer.find(v);
            if (it == producer.end() || dead[it->second] || m.nodes[it->second].op_type != op || graph_outs.count(v)) return -1;
            auto us = users.find(v);
            return us != users.end() && us->second.size() == 1 ? (long)it->second : -1;
        }
        // An Add of two operator outputs is claimed by the LATER producer only (its other operand exists before that producer runs), so two
        // convolutions feeding one Add (projection shortcut + main branch) do not both absorb it.
        bool ready_before(const std::string &v, size_t at) const { auto it = producer.find(v); return it == producer.end() || it->second < at; }
        const std::string &other_input(const onnx::Node &n, const std::string &v) const { return n.inputs[0] == v ? n.inputs[1] : n.inputs[0]; }
        // `node` becomes part of step `st`: it gets no step of its own, the step produces its output and runs where it stood
        void absorb(Step &st, size_t node, std::string &out_name) { dead[node] = true; g.fused_away_++; out_name = m.nodes[node].outputs[0]; st.pos = node; }
    };

    // ---- small questions every step builder asks
    bool is_const(const std::string &v) const { auto it = ids_.find(v); return it != ids_.end() && consts_.count(it->second) != 0; }
    const Tensor &const_of(const std::string &v) const { return consts_.at(ids_.at(v)); }
    bool const_f32_scalar(const std::string &v, float &out) const {
        if (!is_const(v)) return false;
        const Tensor &t = const_of(v);
        if (t.len() != 1 || t.dtype() != DType::F32) return false;
        out = t.to_host<float>()[0];
        return true;
    }
    static std::string label_of(const onnx::Node &n) { return n.name.empty() ? n.outputs.at(0) : n.name; }
    template <class Op> static void run_plainly(Step &st, std::shared_ptr<Op> op) { st.run = [op](Context &c, const InputList &in) { return op->run(c, in); }; }
    // Graph::prepack_weights (src/graph.rs:488-562): a constant weight (input 1) is staged once at load, under the node's label.  `rank`: the one weight rank
    // the operator packs (0: any).  Null: nothing was packed, the step stages its weight per run
    template <class Op> const Tensor *prepacked_weight(const onnx::Node &n, Op &op, bool eligible, int rank) {
        if (!opt_.prepack || !is_const(n.inputs.at(1)) || !eligible) return nullptr;
        const Tensor &w = const_of(n.inputs[1]);
        return rank && w.ndim() != rank ? nullptr : packed_for(label_of(n), [&] { return op.prepack(ctx_, w); });
    }
    // A constant weight zero point (input 3 of ConvInteger / MatMulInteger) that is all zeros (what ort-quantize writes for symmetric weights) is no zero
    // point: dropped at load, the kernel then takes its single-row-term epilogue (integer algebra: the dropped terms are exact zeros).  Measured: 28.1 ->
    // 24.7 us on the dominant launch of the int8 graph -- the whole gap between this executor and the hand-planned runner, which never passed one.
    void drop_zero_zero_point(Step &st) {
        if (!opt_.fuse || st.in[3] < 0 || !consts_.count(st.in[3])) return;
        const Tensor &z = consts_.at(st.in[3]);
        bool all_zero = z.len() > 0 && (z.dtype() == DType::I8 || z.dtype() == DType::U8);
        if (all_zero) for (uint8_t b : z.to_host<uint8_t>()) if (b) { all_zero = false; break; }
        if (all_zero) st.in[3] = -1;
    }
    // (ConvInteger | MatMulInteger) -> Cast(to float) -> Mul(scale): takes the two followers and names the scale.  False: the graph has no such tail
    bool absorb_cast_and_scale(Step &st, Nodes &nodes, std::string &out_name, std::string &scale) {
        const long cast = opt_.fuse ? nodes.sole_user(out_name, "Cast") : -1;
        const long mul = cast >= 0 && nodes[cast].get_int("to", 0) == onnx::FLOAT ? nodes.sole_user(nodes[cast].outputs[0], "Mul") : -1;
        if (mul < 0) return false;
        scale = nodes.other_input(nodes[mul], nodes[cast].outputs[0]);
        nodes.absorb(st, (size_t)cast, out_name);
        nodes.absorb(st, (size_t)mul, out_name);
        return true;
    }
    // keepdims / noop_with_empty_axes / axes of a Reduce* node; axes come from the attribute or (ReduceSum: opset >= 13, the others: opset >= 18) from a constant input
    void read_reduce_attrs(Step &st, const onnx::Node &n, ReduceOp &op) {
        op.keep_dims = n.get_int("keepdims", 1) != 0;
        op.noop_with_empty_axes = n.get_int("noop_with_empty_axes", 0) != 0;
        op.axes = n.get_ints("axes", {});
        if (n.inputs.size() > 1 && !n.inputs[1].empty()) {
            if (!is_const(n.inputs[1])) throw GraphError(n.op_type + " " + st.name + ": the axes input must be a constant");
            for (int32_t v : const_of(n.inputs[1]).to_host<int32_t>()) op.axes.push_back(v);
            st.in.resize(1);
        }
        st.batch_coupled = op.axes.empty() ? !op.noop_with_empty_axes : std::count(op.axes.begin(), op.axes.end(), 0) != 0; // reduces over dim 0
    }
    // An activation node as the kernels' RTEN_HIP_ACT_* kind and parameters, with the reference's attribute defaults (onnx_registry.rs:1132,1228,1275,1999);
    // Clip's min / max come from its opset-6 attributes (promoted to inputs, onnx_registry.rs:887-897) or from constant scalar inputs (an empty name or a
    // missing input: f32::MIN / f32::MAX).  False: not one of these, or a Clip whose bounds are run-time values.
    bool activation_of(const onnx::Node &n, Activation &a) const {
        return activation_of(n, a, [this](const std::string &v, float &out) { return const_f32_scalar(v, out); });
    }
    // (`scalar`: the value of a constant f32 scalar by name, false if it is not one -- the loader's constants, or the initializers of a model that is only parsed)
    static bool activation_of(const onnx::Node &n, Activation &a, const std::function<bool(const std::string &, float &)> &scalar) {
        a = Activation();
        if (n.op_type == "Sigmoid") a.kind = RTEN_HIP_ACT_SIGMOID;
        else if (n.op_type == "Silu") a.kind = RTEN_HIP_ACT_SILU;
        else if (n.op_type == "Swish") { a.kind = RTEN_HIP_ACT_SWISH; a.alpha = n.get_float("alpha", 1.f); }
        else if (n.op_type == "HardSigmoid") { a.kind = RTEN_HIP_ACT_HARD_SIGMOID; a.alpha = n.get_float("alpha", 0.2f); a.beta = n.get_float("beta", 0.5f); }
        else if (n.op_type == "HardSwish") a.kind = RTEN_HIP_ACT_HARD_SWISH;
        else if (n.op_type == "LeakyRelu") { a.kind = RTEN_HIP_ACT_LEAKY_RELU; a.alpha = n.get_float("alpha", 0.01f); }
        else if (n.op_type == "Elu") { a.kind = RTEN_HIP_ACT_ELU; a.alpha = n.get_float("alpha", 1.f); }
        else if (n.op_type == "Clip") {
            a.kind = RTEN_HIP_ACT_CLIP; a.alpha = -FLT_MAX; a.beta = FLT_MAX;
            for (int k = 1; k <= 2; k++) {
                const char *an = k == 1 ? "min" : "max";
                const bool has_in = n.inputs.size() > (size_t)k && !n.inputs[(size_t)k].empty();
                if (n.attr(an) && has_in) throw GraphError("Clip " + n.name + ": input " + std::to_string(k) + " specified as both attribute and input");
                float v = 0.f;
                if (n.attr(an)) v = n.get_float(an, 0.f);
                else if (!has_in) continue;
                else if (!scalar(n.inputs[(size_t)k], v)) return false;
                (k == 1 ? a.alpha : a.beta) = v;
            }
        } else return false;
        return true;
    }

    // ---- attention pre-pass (TransposeFusion + MatMulScale + AddSoftmax of the reference, taken one step further):
    //   q_lin -> Reshape[0,0,h,d] -> Transpose(0,2,1,3) -+
    //   k_lin -> Reshape[0,0,h,d] -> Transpose(0,2,3,1) -+> MatMul -> (Div | Mul scalar) -> Add(mask) -> Softmax(-1) -+
    //   v_lin -> Reshape[0,0,h,d] -> Transpose(0,2,1,3) ------------------------------------------------------------+> MatMul -> Transpose(0,2,1,3) -> Reshape[0,0,H]
    // becomes one MultiHeadSdpa step over the [B, S, H] projections; if the three projections are MatMul(x, W) + Add(b)
    // of one input with constant weights, they become one GEMM against [Wq | Wk | Wv] whose column blocks the
    // attention kernel reads in place (bit-identical: every output element is the same k-ordered dot product).
    // lead0 / lead1: leading dims when the Reshapes spell them out ([B, S, h, d], as PyTorch's exporter writes a static-shape
    // `view`) instead of copying them ([0, 0, h, d]); checked against the projections at run time (0 = copied)
    struct Attn { std::string q, k, v, mask, out, x; int heads = 0; float scale = 1.f; bool merged = false; int wqkv = -1, bqkv = -1; int64_t hidden = 0; int lead0 = 0, lead1 = 0; int head_dim = 0;
                  std::string lead_check; }; // a run-time Reshape target (dynamic-axes export): its leading dims are checked against the projection's when the step runs
    // The matcher: every match is keyed by the node where its step runs (the final Reshape); the nodes it covers are dead from here on.
    std::map<size_t, Attn> plan_attention(Nodes &nodes) {
        const onnx::Model &m = nodes.m;
        std::map<size_t, Attn> attn_at;
        auto const_i32 = [&](const std::string &v, std::vector<int32_t> &out) {
            if (!is_const(v) || const_of(v).dtype() != DType::I32) return false;
            out = const_of(v).to_host<int32_t>();
            return true;
        };
        auto leading_ok = [](const std::vector<int32_t> &shp, Attn &at, bool first) { // [0, 0, ..] or one explicit [B, S, ..] throughout
            if ((shp[0] == 0) != (shp[1] == 0) || shp[0] < 0 || shp[1] < 0) return false;
            if (first) { at.lead0 = shp[0]; at.lead1 = shp[1]; return true; }
            return at.lead0 == shp[0] && at.lead1 == shp[1];
        };
        // The target of a head-split / head-merge Reshape: a constant, or -- exports with dynamic axes -- Concat(dim 0, dim 1, [h | -1], [d]) whose leading
        // entries are computed from a Shape at run time and whose trailing entries are constants.  The run-time form reads as [0, 0, ..] ("copy the
        // projection's leading dims"); `dyn` names the Concat's output so that the fused step can check that claim against its host value.
        auto reshape_target = [&](const onnx::Node &rn, std::vector<int32_t> &shp, std::string &dyn) {
            dyn.clear();
            if (rn.inputs.size() < 2) return false;
            if (const_i32(rn.inputs[1], shp)) return true;
            const long c = nodes.made_by(rn.inputs[1], "Concat");
            if (c < 0 || nodes[c].get_int("axis", 0) != 0 || nodes[c].inputs.size() < 3) return false;
            const onnx::Node &cn = nodes[c];
            shp.assign(cn.inputs.size(), 0);
            for (size_t k = 0; k < cn.inputs.size(); k++) {
                std::vector<int32_t> one;
                if (k < 2) { if (is_const(cn.inputs[k])) return false; continue; } // (a half-constant leading pair is not this idiom)
                if (!const_i32(cn.inputs[k], one) || one.size() != 1) return false;
                shp[k] = one[0];
            }
            dyn = rn.inputs[1];
            return true;
        };
        // value -> (Reshape[0,0,h,d] node, Transpose node) feeding it with the given perm; returns the projection's name
        auto split_heads = [&](const std::string &v, std::vector<int> perm, Attn &at, bool first, std::vector<size_t> &covered) -> std::string {
            int &heads = at.heads;
            const long t = nodes.made_by(v, "Transpose");
            if (t < 0 || nodes[t].get_ints("perm", {}) != perm) return "";
            const long r = nodes.made_by(nodes[t].inputs[0], "Reshape");
            std::vector<int32_t> shp;
            std::string dyn;
            // [.., .., h, d] or [.., .., -1, d]: transformers' exporter spells the head COUNT as -1 (hidden / d, resolved when the step runs)
            if (r < 0 || !reshape_target(nodes[r], shp, dyn) || shp.size() != 4 || (shp[2] <= 0 && !(shp[2] == -1 && shp[3] > 0)) || !leading_ok(shp, at, first)) return "";
            if (first) at.lead_check = dyn;
            if (heads && heads != shp[2]) return "";
            // one head size for q, k and v (the kernel's d == dv); -1 ("the rest") is accepted only if all three say so
            if (heads && at.head_dim != shp[3]) return "";
            heads = shp[2];
            at.head_dim = shp[3];
            covered.push_back((size_t)t); covered.push_back((size_t)r);
            return nodes[r].inputs[0];
        };
        // a projection written as MatMul(x, W constant [K, N]) + Add(b constant [N]), either operand order
        struct Lin { long mm = -1, add = -1; std::string x, w, b; };
        auto linear = [&](const std::string &v) {
            Lin l;
            const long a = nodes.made_by(v, "Add");
            if (a < 0) return l;
            for (int side = 0; side < 2; side++) {
                const std::string &mmv = nodes[a].inputs[(size_t)side], &bv = nodes[a].inputs[(size_t)(1 - side)];
                const long mmi = nodes.made_by(mmv, "MatMul");
                if (mmi < 0 || !is_const(bv) || !is_const(nodes[mmi].inputs[1])) continue;
                const Tensor &w = const_of(nodes[mmi].inputs[1]), &b = const_of(bv);
                if (w.ndim() != 2 || b.ndim() != 1 || b.len() != w.size(1) || w.dtype() != DType::F32 || b.dtype() != DType::F32) continue;
                l.mm = mmi; l.add = a; l.x = nodes[mmi].inputs[0]; l.w = nodes[mmi].inputs[1]; l.b = bv;
                return l;
            }
            return l;
        };
        for (size_t i = 0; i < m.nodes.size(); i++) {
            const onnx::Node &mm = m.nodes[i];
            if (nodes.dead[i] || mm.op_type != "MatMul" || mm.inputs.size() != 2) continue;
            Attn at;
            std::vector<size_t> covered{i};
            at.q = split_heads(mm.inputs[0], {0, 2, 1, 3}, at, true, covered);
            at.k = at.q.empty() ? "" : split_heads(mm.inputs[1], {0, 2, 3, 1}, at, false, covered);
            if (at.k.empty()) continue;
            std::string cur = mm.outputs[0];
            for (const char *sop : {"Div", "Mul"}) {
                const long d = nodes.sole_user(cur, sop);
                float cv = 0.f;
                if (d < 0 || at.scale != 1.f || nodes[d].inputs.size() != 2 || nodes[d].inputs[0] == nodes[d].inputs[1]) continue;
                const bool div = std::string(sop) == "Div";
                if (nodes[d].inputs[0] != cur && div) continue; // Mul takes the scalar on either side, Div on the right only (MatMulScaleFusion, fusions.rs:884-906)
                if (!const_f32_scalar(nodes.other_input(nodes[d], cur), cv)) continue;
                at.scale = div ? 1.0f / cv : cv;
                covered.push_back((size_t)d);
                cur = nodes[d].outputs[0];
            }
            const long add = nodes.sole_user(cur, "Add");
            if (add >= 0) { at.mask = nodes.other_input(nodes[add], cur); covered.push_back((size_t)add); cur = nodes[add].outputs[0]; }
            const long sm = nodes.sole_user(cur, "Softmax");
            const int64_t sm_axis = sm < 0 ? 0 : nodes[sm].get_int("axis", -1);
            if (sm < 0 || (sm_axis != -1 && sm_axis != 3)) continue; // the scores are 4-D here: PyTorch's exporter writes the last axis as 3
            covered.push_back((size_t)sm);
            cur = nodes[sm].outputs[0];
            const long pv = nodes.sole_user(cur, "MatMul");
            if (pv < 0 || nodes[pv].inputs[0] != cur) continue;
            covered.push_back((size_t)pv);
            at.v = split_heads(nodes[pv].inputs[1], {0, 2, 1, 3}, at, false, covered);
            if (at.v.empty()) continue;
            const long tr = nodes.sole_user(nodes[pv].outputs[0], "Transpose");
            if (tr < 0 || nodes[tr].get_ints("perm", {}) != std::vector<int>{0, 2, 1, 3}) continue;
            const long rs = nodes.sole_user(nodes[tr].outputs[0], "Reshape");
            std::vector<int32_t> shp;
            std::string dyn_out;
            if (rs < 0 || !reshape_target(nodes[rs], shp, dyn_out) || shp.size() != 3 || !leading_ok(shp, at, false)) continue;
            covered.push_back((size_t)tr); covered.push_back((size_t)rs);
            at.out = nodes[rs].outputs[0];
            if (!at.mask.empty() && !nodes.ready_before(at.mask, i + 1)) continue; // mask must exist before the scores
            if (!at.mask.empty() && is_const(at.mask)) { // a constant mask with a head axis is outside the kernel's forms: leave the graph unfused
                const Tensor &mk = const_of(at.mask);
                if (mk.dtype() != DType::F32 || mk.ndim() > 4 || (mk.ndim() == 4 && mk.size(1) != 1) || (mk.ndim() == 3 && mk.size(0) != 1)) continue;
            }
            // optional: one GEMM for the three projections
            const Lin lq = linear(at.q), lk = linear(at.k), lv = linear(at.v);
            const bool one_input = lq.mm >= 0 && lk.mm >= 0 && lv.mm >= 0 && lq.x == lk.x && lq.x == lv.x;
            if (one_input && const_of(lq.w).shape() == const_of(lk.w).shape() && const_of(lq.w).shape() == const_of(lv.w).shape()) {
                const Tensor &wq = const_of(lq.w), &wk = const_of(lk.w), &wv = const_of(lv.w);
                const int64_t K = wq.size(0), Nn = wq.size(1);
                const std::vector<float> hq = wq.to_host<float>(), hk = wk.to_host<float>(), hv = wv.to_host<float>();
                std::vector<float> wcat((size_t)(K * 3 * Nn)), bcat;
                for (int64_t r = 0; r < K; r++) {
                    std::copy(hq.begin() + r * Nn, hq.begin() + (r + 1) * Nn, wcat.begin() + r * 3 * Nn);
                    std::copy(hk.begin() + r * Nn, hk.begin() + (r + 1) * Nn, wcat.begin() + r * 3 * Nn + Nn);
                    std::copy(hv.begin() + r * Nn, hv.begin() + (r + 1) * Nn, wcat.begin() + r * 3 * Nn + 2 * Nn);
                }
                for (const std::string *bn : {&lq.b, &lk.b, &lv.b}) { const std::vector<float> hb = const_of(*bn).to_host<float>(); bcat.insert(bcat.end(), hb.begin(), hb.end()); }
                at.wqkv = id_of("__qkv_w." + std::to_string(i));
                at.bqkv = id_of("__qkv_b." + std::to_string(i));
                add_const(at.wqkv, [&] { return Tensor::from_host<float>(ctx_, {K, 3 * Nn}, wcat.data()); });
                add_const(at.bqkv, [&] { return Tensor::from_host<float>(ctx_, {3 * Nn}, bcat.data()); });
                at.merged = true; at.x = lq.x; at.hidden = Nn;
                for (long d : {lq.mm, lq.add, lk.mm, lk.add, lv.mm, lv.add}) covered.push_back((size_t)d);
            }
            for (size_t d : covered) nodes.dead[d] = true;
            fused_away_ += covered.size() - (at.merged ? 2 : 1);
            attn_at[(size_t)rs] = at;
        }
        return attn_at;
    }
    // The step(s) of one match, at node `pos`: MultiHeadSdpa, after one FusedMatMul for the three projections when they were merged.
    void emit_attention(const Attn &at, size_t pos) {
        auto op = std::make_shared<MultiHeadSdpa>();
        op->heads = at.heads; op->head_dim = at.head_dim; op->scale = at.scale; op->flush_nans_to_zero = false;
        Step st;
        st.pos = pos;
        st.name = at.out;
        st.kind_name = at.merged ? "MultiHeadSdpa(QKV column blocks)" : "MultiHeadSdpa";
        if (at.merged) {
            auto lin = std::make_shared<FusedMatMul>();
            Step pj;
            pj.pos = pos;
            pj.name = at.out + ".qkv";
            pj.kind_name = "FusedMatMul(QKV)";
            pj.in = {id_of(at.x), at.wqkv, at.bqkv};
            const int qkv = id_of("__qkv." + at.out);
            pj.out = {qkv};
            auto plan = std::make_shared<GemmPlan>();
            pj.gemm_plan = plan;
            pj.run = [lin, plan](Context &c, const InputList &in) { PlanScope scope(c, *plan); return lin->run(c, in); };
            steps_.push_back(std::move(pj));
            op->q_rs = op->k_rs = op->v_rs = 3 * at.hidden; op->width = at.hidden;
            op->q_off = 0; op->k_off = at.hidden; op->v_off = 2 * at.hidden;
            st.in = {qkv, qkv, qkv, at.mask.empty() ? -1 : id_of(at.mask)};
        } else {
            st.in = {id_of(at.q), id_of(at.k), id_of(at.v), at.mask.empty() ? -1 : id_of(at.mask)};
        }
        st.out = {id_of(at.out)};
        if (!at.lead_check.empty()) st.in.push_back(id_of(at.lead_check)); // (5th operand: the run-time Reshape target, a host value)
        const int lead0 = at.lead0, lead1 = at.lead1;
        // A run-time mask with a head axis ([B | 1, H, S, T]: a relative-position or per-head bias fed as an input) is outside the kernel's forms, and the plan
        // cannot know it: the step then runs the operators it covers plainly, in graph order -- head-split views, Transpose, MatMul with the scale as
        // FusedMatMul's alpha (MatMulScaleFusion), Add, Softmax, MatMul, Transpose, head-merge view -- which are the interpreter's bits.  Launches only: capture-safe.
        auto plain = [op](Context &c, const InputList &in) {
            const Tensor &q = require(in, 0), &k = require(in, 1), &v = require(in, 2);
            if (q.ndim() != 3 || k.ndim() != 3 || v.ndim() != 3) throw OpError(OpError::InvalidValue, "expected [batch, seq, hidden] projections");
            const int64_t B = q.size(0), S = q.size(1), T = k.size(1), Hd = op->width ? op->width : q.size(2);
            const int64_t heads = op->heads > 0 ? op->heads : (op->head_dim > 0 && Hd % op->head_dim == 0 ? Hd / op->head_dim : 0);
            if (heads <= 0 || Hd % heads != 0) throw OpError(OpError::InvalidValue, "hidden size is not divisible by the number of heads");
            if (k.size(0) != B || v.size(0) != B || v.size(1) != T || (!op->width && (k.size(2) != Hd || v.size(2) != Hd)))
                throw OpError(OpError::IncompatibleInputShapes, "q / k / v batch, sequence or hidden sizes do not match");
            const int64_t d = Hd / heads;
            auto split = [&](const Tensor &t, int64_t off, std::vector<int> perm) { // a column block of the merged projection is sliced out first
                Tensor block = op->width ? slice_tensor(c, t, {{0, t.size(0), 1}, {0, t.size(1), 1}, {off, Hd, 1}}) : Tensor::view_of(t, t.shape());
                const Tensor heads4 = Tensor::view_of(block, {t.size(0), t.size(1), heads, d});
                Transpose tr;
                tr.perm = std::move(perm);
                return tr.run(c, {&heads4});
            };
            const OutputList qh = split(q, op->q_off, {0, 2, 1, 3}), kh = split(k, op->k_off, {0, 2, 3, 1}), vh = split(v, op->v_off, {0, 2, 1, 3});
            FusedMatMul qk;
            qk.alpha = op->scale;
            const OutputList scores = qk.run(c, {&qh[0], &kh[0]});
            const OutputList sum = Add().run(c, {&scores[0], &require(in, 3)});
            const OutputList probs = Softmax().run(c, {&sum[0]});
            const OutputList ctx4 = MatMul().run(c, {&probs[0], &vh[0]});
            Transpose back;
            back.perm = {0, 2, 1, 3};
            OutputList out = back.run(c, {&ctx4[0]});
            out[0].reshape({B, S, Hd});
            return out;
        };
        auto run_attention = [op, plain](Context &c, const InputList &in) {
            const Tensor *mask = in.size() > 3 ? in[3] : nullptr;
            const bool head_axis = mask && mask->ndim() >= 3 && mask->ndim() <= 4 && mask->size(mask->ndim() - 3) != 1;
            return head_axis ? plain(c, in) : op->run(c, in);
        };
        st.run = [run_attention, lead0, lead1](Context &c, const InputList &in) {
            if (lead0 && (require(in, 0).ndim() != 3 || require(in, 0).size(0) != lead0 || require(in, 0).size(1) != lead1))
                throw OpError(OpError::InvalidValue, "fused attention: the graph's Reshape spells out leading dims that differ from the projection's");
            if (in.size() > 4 && in[4]) { // the Reshape target the graph computes at run time must say what the fusion assumed: [B, S, ..] of the projection
                const std::vector<int64_t> tgt = host_ints(in[4], "fused attention: the head-split Reshape's target");
                if (require(in, 0).ndim() != 3 || tgt.size() != 4 || tgt[0] != require(in, 0).size(0) || tgt[1] != require(in, 0).size(1))
                    throw OpError(OpError::InvalidValue, "fused attention: the graph's Reshape target differs from the projection's leading dims");
                return run_attention(c, InputList(in.begin(), in.begin() + 4));
            }
            return run_attention(c, in);
        };
        steps_.push_back(std::move(st));
    }

    // ---- compile: constants, the attention pre-pass, one step per remaining node (the make_*_step members below, each with the followers it absorbs), then
    //      the step-level passes and liveness
    void compile(const onnx::Model &m_in) {
        const onnx::Model m = canonicalize(m_in);
        inputs_ = m.inputs;
        outputs_ = m.outputs;
        for (auto &t : m.initializers) add_const(id_of(t.name), [&] { return upload(t); });
        for (auto &in : m.inputs) id_of(in.name);

        Nodes nodes(*this, m);
        const std::map<size_t, Attn> attn_at = opt_.fuse ? plan_attention(nodes) : std::map<size_t, Attn>();
        for (size_t i = 0; i < m.nodes.size(); i++) {
            auto af = attn_at.find(i);
            if (af != attn_at.end()) { emit_attention(af->second, i); continue; }
            if (nodes.dead[i]) continue;
            const onnx::Node &n = m.nodes[i];
            // contrib operators this backend carries live in com.microsoft (onnx_registry.rs registers them under that domain)
            const bool contrib = n.domain == "com.microsoft" && (n.op_type == "MatMulNBits" || is_decoder_node(n) || is_gqa_node(n));
            if (!n.domain.empty() && n.domain != "ai.onnx" && !contrib) throw GraphError("node " + n.name + ": operator domain " + n.domain + " is not supported");
            Step st;
            st.name = label_of(n);
            st.kind_name = n.op_type;
            st.pos = i;
            for (auto &s : n.inputs) st.in.push_back(id_of(s));
            std::string out_name = n.outputs.at(0); // becomes the output of the last node the step absorbs

            const std::string &kind = n.op_type;
            if (kind == "Conv") make_conv_step(st, n, nodes, out_name);
            else if (kind == "ConvTranspose") {
                auto op = std::make_shared<ConvTranspose>();
                op->groups = (int)n.get_int("group", 1);
                op->strides = n.get_ints("strides", {1, 1});
                op->dilations = n.get_ints("dilations", {1, 1});
                op->output_padding = n.get_ints("output_padding", {});
                op->padding = padding_of(n, "ConvTranspose");
                if (n.attr("output_shape")) throw GraphError("ConvTranspose " + st.name + ": the output_shape attribute is not supported");
                run_plainly(st, op);
            } else if (kind == "MatMulNBits") { // com.microsoft contrib op (onnx_registry reads bits / block_size / accuracy_level)
                auto op = std::make_shared<MatMulNBits>();
                op->bits = (int)n.get_int("bits", 4);
                op->block_size = n.get_int("block_size", 32);
                op->accuracy_level = (int)n.get_int("accuracy_level", 0);
                run_plainly(st, op);
            } else if (kind == "ConvInteger") make_conv_integer_step(st, n, nodes, out_name);
            else if (kind == "MatMulInteger") make_matmul_integer_step(st, n, nodes, out_name);
            else if (kind == "Gemm") {
                auto op = std::make_shared<Gemm>();
                op->alpha = n.get_float("alpha", 1.f); op->beta = n.get_float("beta", 1.f);
                op->transpose_a = n.get_int("transA", 0) != 0; op->transpose_b = n.get_int("transB", 0) != 0;
                auto plan = std::make_shared<GemmPlan>();
                st.gemm_plan = plan;
                st.run = [op, plan](Context &c, const InputList &in) { PlanScope scope(c, *plan); return op->run(c, in); };
            } else if (kind == "MatMul") make_matmul_step(st, n, nodes, out_name);
            else if (kind == "Add" && opt_.fuse && make_add_norm_step(st, n, nodes, out_name)) {} // (any other Add takes the generic path below)
            else if (is_gqa_node(n)) make_gqa_step(st, n, m);
            else if (is_decoder_node(n)) make_decoder_step(st, n, m); // (RotaryEmbedding dispatches on its domain, the skip forms exist in com.microsoft only)
            else if (kind == "LayerNormalization") {
                auto op = std::make_shared<LayerNormalization>();
                op->axis = (int)n.get_int("axis", -1);
                op->epsilon = n.get_float("epsilon", 1e-5f);
                st.batch_coupled = op->axis == 0;
                const std::string nm = st.name;
                st.run = [this, op, nm](Context &c, const InputList &in) { note_axis("LayerNormalization", nm, op->axis, require(in, 0)); return op->run(c, in); };
            } else if (kind == "Sigmoid" || kind == "Silu" || kind == "Swish" || kind == "HardSigmoid" || kind == "HardSwish" || kind == "LeakyRelu" || kind == "Elu" || kind == "Clip")
                make_activation_step(st, n);
            else if (kind == "Gelu" && n.attr("approximate") && n.attr("approximate")->s != "none")
                throw GraphError("Gelu " + st.name + ": approximate=\"" + n.attr("approximate")->s + "\" is not supported");
            else if (kind == "MaxPool" || kind == "AveragePool") make_pool_step(st, n);
            else if (kind == "Einsum") {
                auto op = std::make_shared<Einsum>();
                if (!n.attr("equation")) throw GraphError("Einsum " + st.name + ": the equation attribute is missing");
                op->equation = n.attr("equation")->s;
                run_plainly(st, op);
            } else if (kind == "ReduceSum" || kind == "ReduceMean" || kind == "ReduceMax" || kind == "ReduceMin" || reduce_family_kind(kind) >= 0) make_reduce_step(st, n);
            else if (kind == "LpNormalization") {
                const LpNormNode a = read_lp_norm_node(n, st.name);
                auto op = std::make_shared<LpNormalization>();
                op->axis = a.axis;
                op->p = a.p;
                st.batch_coupled = op->axis == 0; // (a negative axis that resolves to dim 0 is a run-time fact: note_axis)
                const std::string nm = st.name;
                st.run = [this, op, nm](Context &c, const InputList &in) { note_axis("LpNormalization", nm, op->axis, require(in, 0)); return op->run(c, in); };
            } else if (kind == "GlobalMaxPool") run_plainly(st, std::make_shared<GlobalMaxPool>()); // per (n, c) plane: rows of the batch are independent
            else if (kind == "GridSample") { // per batch row (the grid's dim 0 is the input's); one launch, nothing read back, no shape from data
                auto op = std::make_shared<GridSample>();
                op->align_corners = read_grid_sample_node(n, st.name).align_corners;
                run_plainly(st, op);
            } else if (kind == "DepthToSpace") { // a permutation inside every batch row: one transpose launch
                const DepthToSpaceNode a = read_depth_to_space_node(n, st.name);
                auto op = std::make_shared<DepthToSpace>();
                op->block_size = a.block_size;
                op->mode = a.mode;
                run_plainly(st, op);
            }
            else if (kind == "ArgMax" || kind == "ArgMin" || kind == "TopK" || kind == "Softmax") make_select_step(st, n);
            else if (kind == "Resize" || kind == "Upsample") make_resize_step(st, n);
            else if (kind == "Split") make_split_step(st, n);
            else if (kind == "GRU" || kind == "LSTM") make_rnn_step(st, n);
            else if (kind == "InstanceNormalization" || kind == "BatchNormalization" || kind == "LogSoftmax") make_norm_step(st, n, nodes, out_name);
            else if (is_math_kind(kind)) make_math_step(st, n, m);
            else if (kind == "Pad") make_pad_step(st, n, m);
            else if (is_index_kind(kind)) make_index_step(st, n, m);
            else if (kind == "NonMaxSuppression") make_nms_step(st, n, m);
            else if (kind == "DFT" || kind == "STFT") make_fft_step(st, n, m);
            else if (kind == "QuantizeLinear" || kind == "DequantizeLinear") make_qdq_step(st, n, m, nodes, out_name);
            else if (kind == "Flatten" || kind == "Reshape" || kind == "Squeeze" || kind == "Unsqueeze" || kind == "Identity" || kind == "Dropout") make_view_step(st, n);
            else if (make_layout_step(st, n)) {
                // Shape / ConstantOfShape / NonZero / Range / Slice / Concat / Expand / Where / comparisons / logic / integer arithmetic / Cast / Gather /
                // Transpose: host-evaluated when their operands are host values, device kernels otherwise
            } else {
                static const OpRegistry reg = OpRegistry::with_all_ops();
                if (!reg.contains(kind)) throw GraphError("node " + st.name + ": operator " + kind + " is not available on the HIP backend (no CPU fallback)");
                run_plainly(st, std::shared_ptr<Operator>(reg.create(kind).release()));
            }
            st.out.push_back(id_of(out_name));
            for (size_t k = 1; k < n.outputs.size(); k++) st.out.push_back(n.outputs[k].empty() ? -1 : id_of(n.outputs[k]));
            if (st.extra_out >= 0) st.out.push_back(st.extra_out);
            steps_.push_back(std::move(st));
        }
        for (auto &o : m.outputs)
            if (!ids_.count(o.name)) throw GraphError("graph output " + o.name + " is not produced by any node");
        std::stable_sort(steps_.begin(), steps_.end(), [](const Step &a, const Step &b) { return a.pos < b.pos; });
        for (auto &st : steps_) if (st.view && st.out[0] >= 0) view_values_.insert(st.out[0]);
        if (opt_.fuse) { plan_int8_staging(); plan_dql_loaders(); plan_conv_pairs(); }
        for (auto &st : steps_) if (st.kind_name.find("DynamicQuantizeLinear") != std::string::npos) st.batch_coupled = true; // min / max over the whole tensor
        plan_liveness();
    }

    // Conv (+ Add residual) (+ Relu, or one activation activation_of takes)
    void make_conv_step(Step &st, const onnx::Node &n, Nodes &nodes, std::string &out_name) {
        auto op = std::make_shared<Conv>(conv_attrs(n, n.inputs.size() > 1 && is_const(n.inputs[1]) ? const_of(n.inputs[1]).ndim() : 0));
        const size_t at = st.pos;
        std::string residual;
        if (opt_.fuse) {
            const long a = nodes.sole_user(out_name, "Add");
            if (a >= 0 && nodes[a].inputs.size() == 2) {
                const std::string other = nodes.other_input(nodes[a], out_name);
                if (other != out_name && nodes.ready_before(other, at)) { residual = other; nodes.absorb(st, (size_t)a, out_name); }
            }
            const long r = nodes.sole_user(out_name, "Relu");
            if (r >= 0) { op->fuse_relu = true; nodes.absorb(st, (size_t)r, out_name); }
            Activation act;
            const long ac = op->fuse_relu ? -1 : nodes.sole_activation(out_name, act);
            if (ac >= 0) { op->act = act; nodes.absorb(st, (size_t)ac, out_name); }
        }
        while (st.in.size() < 3) st.in.push_back(-1);
        st.in.push_back(residual.empty() ? -1 : id_of(residual));
        const Tensor *packed = prepacked_weight(n, *op, op->groups == 1, 4);
        st.kind_name = std::string("Conv") + (residual.empty() ? "" : "+Add") + (op->fuse_relu ? "+Relu" : "") +
                       (op->act.kind != RTEN_HIP_ACT_NONE ? std::string("+") + activation_name(op->act.kind) : "");
        st.conv = op;
        // The Add's other operand is used as the kernel's residual only when it has exactly the conv's output shape
        // (the kernel indexes it with the output's strides).  Its shape is a run-time fact (no shape inference here), and
        // it may be a constant or any broadcasting operand -- e.g. the exporter's explicit bias Add([1,O,1,1]) -- so a
        // mismatch runs the operators as the graph spells them: Conv, broadcasting Add, Relu.  (The constant is NOT
        // routed to the conv's bias input: the GEMM adds a bias after the first depth block, the graph adds it last.)
        st.run = [op, packed](Context &c, const InputList &in) {
            const Tensor *res = in.size() > 3 ? in[3] : nullptr;
            if (res) {
                const Tensor &x = require(in, 0), &w = require(in, 1);
                bool same = res->dtype() == DType::F32 && x.ndim() == 4 && w.ndim() == 4; // 1-D convs with an Add: always unfused
                if (same) {
                    const rten_hip_conv2d_desc d = op->geometry(x.shape(), w.shape());
                    same = res->shape() == std::vector<int64_t>{d.n, d.o, d.out_h, d.out_w};
                }
                if (!same) {
                    Conv plain = *op; plain.fuse_relu = false; plain.act = Activation();
                    OutputList y = plain.run_packed(c, {in[0], in[1], in.size() > 2 ? in[2] : nullptr}, packed);
                    OutputList sum = Add().run(c, {&y[0], res});
                    if (op->act.kind != RTEN_HIP_ACT_NONE) return ActivationOp(op->act.kind, op->act.alpha, op->act.beta).run(c, {&sum[0]});
                    return op->fuse_relu ? Relu().run(c, {&sum[0]}) : std::move(sum);
                }
            }
            return op->run_packed(c, in, packed);
        };
    }
    // ConvInteger -> Cast -> Mul(scale) (= ConvIntegerToFloat) (+ Add bias constant [1, O, 1, 1]) (+ Add residual) (+ Relu)
    void make_conv_integer_step(Step &st, const onnx::Node &n, Nodes &nodes, std::string &out_name) {
        auto op = std::make_shared<ConvInteger>();
        op->conv = conv_attrs(n);
        const size_t at = st.pos;
        std::string scale, bias, residual;
        bool relu = false;
        // ConvIntegerToFloat: the Mul's other operand must be a single scale available before the conv runs
        if (absorb_cast_and_scale(st, nodes, out_name, scale)) {
            const long add = nodes.sole_user(out_name, "Add");
            if (add >= 0) { // Add(bias constant [1, O, 1, 1])
                const std::string b = nodes.other_input(nodes[add], out_name);
                if (is_const(b)) {
                    const Tensor &bt = const_of(b);
                    if (bt.ndim() == 4 && bt.size(0) == 1 && bt.size(2) == 1 && bt.size(3) == 1) { bias = b; nodes.absorb(st, (size_t)add, out_name); }
                }
            }
            const long add2 = bias.empty() ? -1 : nodes.sole_user(out_name, "Add");
            if (add2 >= 0) {
                const std::string other = nodes.other_input(nodes[add2], out_name);
                if (other != out_name && nodes.ready_before(other, at)) { residual = other; nodes.absorb(st, (size_t)add2, out_name); }
            }
            const long r = nodes.sole_user(out_name, "Relu");
            if (r >= 0) { relu = true; nodes.absorb(st, (size_t)r, out_name); }
        }
        while (st.in.size() < 4) st.in.push_back(-1);
        drop_zero_zero_point(st);
        st.in.push_back(scale.empty() ? -1 : id_of(scale));
        st.in.push_back(bias.empty() ? -1 : id_of(bias));
        st.in.push_back(residual.empty() ? -1 : id_of(residual));
        if (!scale.empty()) st.kind_name = std::string("ConvIntegerToFloat") + (bias.empty() ? "" : "+bias") + (residual.empty() ? "" : "+Add") + (relu ? "+Relu" : "");
        auto state = std::make_shared<I8Conv>();
        state->op = op;
        state->to_float = !scale.empty();
        state->sg.packed_weight = prepacked_weight(n, *op, op->conv.groups == 1, 4);
        st.i8 = state;
        // ConvIntegerToFloatFusion (fusions.rs:1012-1058) fuses only a scale of shape [] or [1] and leaves every other graph
        // as ConvInteger -> Cast -> Mul.  Shapes are run-time facts here, so the step decides per run: a scalar f32 scale
        // (or a per-output-channel [1,O,1,1] / [O,1,1] one, which the kernel applies exactly as Cast -> Mul would) with a
        // bias of O channels and a residual of the output's shape takes the fused kernel; anything else runs the
        // operators as the graph spells them.
        state->relu = relu;
        st.run = [state, relu](Context &c, const InputList &in) {
            const Tensor *scale = in[4], *bias = in[5], *residual = in[6];
            if (!scale) return state->op->run_staged(c, InputList(in.begin(), in.begin() + 4), nullptr, nullptr, nullptr, false, state->sg);
            bool per_channel = false;
            const bool fused = i8_fused_form(*state, in, per_channel);
            if (fused) return state->op->run_staged(c, InputList(in.begin(), in.begin() + 4), scale, bias, residual, relu, state->sg, per_channel);
            ConvInteger::Staging sg = state->sg;
            sg.stats_out = nullptr; // statistics are accumulated by the float epilogue only
            OutputList acc = state->op->run_staged(c, InputList(in.begin(), in.begin() + 4), nullptr, nullptr, nullptr, false, sg);
            Cast cast; cast.to = DType::F32;
            OutputList f = cast.run(c, {&acc[0]});
            OutputList y = Mul().run(c, {&f[0], scale});
            if (bias) y = Add().run(c, {&y[0], bias});
            if (residual) y = Add().run(c, {&y[0], residual});
            if (relu) y = Relu().run(c, {&y[0]});
            return y;
        };
    }
    // MatMulInteger -> Cast -> Mul(scale) (= MatMulIntegerToFloat)
    void make_matmul_integer_step(Step &st, const onnx::Node &n, Nodes &nodes, std::string &out_name) {
        auto op = std::make_shared<MatMulInteger>();
        std::string scale;
        absorb_cast_and_scale(st, nodes, out_name, scale);
        while (st.in.size() < 4) st.in.push_back(-1);
        drop_zero_zero_point(st);
        st.in.push_back(scale.empty() ? -1 : id_of(scale));
        if (!scale.empty()) st.kind_name = "MatMulIntegerToFloat";
        const Tensor *packed = prepacked_weight(n, *op, true, 0); // a constant RHS (PackedBMatrix)
        // MatMulIntegerToFloatFusion (fusions.rs:960-1009) needs a scale of rank <= 1; the operator then needs length 1 or N.
        // Decided per run (shapes are run-time facts); otherwise MatMulInteger -> Cast -> Mul as the graph spells it.
        st.run = [op, packed](Context &c, const InputList &in) {
            const Tensor *scale = in[4];
            if (scale) {
                const Tensor &b = require(in, 1);
                const int64_t ncols = b.ndim() > 1 ? b.size(b.ndim() - 1) : 1;
                const bool ok = scale->dtype() == DType::F32 && scale->ndim() <= 1 && (scale->len() == 1 || scale->len() == ncols);
                if (!ok) {
                    OutputList acc = op->run_scaled(c, InputList(in.begin(), in.begin() + 4), nullptr, packed);
                    Cast cast; cast.to = DType::F32;
                    OutputList f = cast.run(c, {&acc[0]});
                    return Mul().run(c, {&f[0], scale});
                }
            }
            return op->run_scaled(c, InputList(in.begin(), in.begin() + 4), scale, packed);
        };
    }
    // MatMul (+ Mul / Div by a constant scalar = alpha, MatMulScale fusion) (+ Add of a constant 1-D bias,
    // MatMulAddFusion) (+ Gelu / Relu as the GEMM epilogue): FusedMatMul (src/ops/matmul.rs:455-510)
    void make_matmul_step(Step &st, const onnx::Node &, Nodes &nodes, std::string &out_name) {
        auto op = std::make_shared<FusedMatMul>();
        std::string bias;
        if (opt_.fuse) {
            for (const char *sop : {"Div", "Mul"}) {
                const long d = nodes.sole_user(out_name, sop);
                const bool div = std::string(sop) == "Div";
                float c = 0.f;
                if (d < 0 || nodes[d].inputs.size() != 2 || op->alpha != 1.f) continue;
                // the product on the left and the scalar on the right, or -- Mul only -- the other way round (get_scale_factor, fusions.rs:884-906)
                const bool right = nodes[d].inputs[0] == out_name && const_f32_scalar(nodes[d].inputs[1], c);
                const bool left = !right && !div && nodes[d].inputs[1] == out_name && const_f32_scalar(nodes[d].inputs[0], c);
                if (right || left) {
                    op->alpha = div ? 1.0f / c : c;
                    nodes.absorb(st, (size_t)d, out_name);
                }
            }
            const long a = op->alpha == 1.f ? nodes.sole_user(out_name, "Add") : -1;
            if (a >= 0) {
                const std::string other = nodes.other_input(nodes[a], out_name);
                if (is_const(other) && const_of(other).ndim() == 1 && const_of(other).dtype() == DType::F32) {
                    bias = other;
                    nodes.absorb(st, (size_t)a, out_name);
                    const long g = nodes.sole_user(out_name, "Gelu");
                    if (g >= 0 && !nodes[g].attr("approximate")) { op->act = RTEN_HIP_ACT_GELU; nodes.absorb(st, (size_t)g, out_name); }
                    const long r = g < 0 ? nodes.sole_user(out_name, "Relu") : -1;
                    if (r >= 0) { op->act = RTEN_HIP_ACT_RELU; nodes.absorb(st, (size_t)r, out_name); }
                }
            }
            Activation act;
            const long ac = op->act == RTEN_HIP_ACT_NONE ? nodes.sole_activation(out_name, act) : -1;
            if (ac >= 0) { op->act = act.kind; op->act_alpha = act.alpha; op->act_beta = act.beta; nodes.absorb(st, (size_t)ac, out_name); }
        }
        st.in.resize(2);
        st.in.push_back(bias.empty() ? -1 : id_of(bias));
        st.kind_name = std::string(op->alpha != 1.f || !bias.empty() || op->act > RTEN_HIP_ACT_GELU ? "FusedMatMul" : "MatMul") +
                       (op->act != RTEN_HIP_ACT_NONE ? std::string("+") + activation_name(op->act) : "");
        auto plan = std::make_shared<GemmPlan>();
        st.gemm_plan = plan;
        st.run = [op, plan](Context &c, const InputList &in) {
            const Tensor *bias = in[2];
            if (bias && bias->len() != require(in, 1).size(require(in, 1).ndim() - 1)) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast bias to output shape");
            PlanScope scope(c, *plan);
            return op->run(c, in);
        };
    }
    // The two fused forms of Add, tried before the generic path.  False: this Add is neither.
    bool make_add_norm_step(Step &st, const onnx::Node &, Nodes &nodes, std::string &out_name) {
        const long ln = nodes.sole_user(out_name, "LayerNormalization");
        if (ln >= 0 && nodes[ln].get_int("axis", -1) == -1 && nodes[ln].inputs[0] == out_name) {
            // Add(residual) -> LayerNormalization(last axis) as one kernel
            const onnx::Node &lnn = nodes[ln];
            auto fused = std::make_shared<AddLayerNormalization>();
            fused->epsilon = lnn.get_float("epsilon", 1e-5f);
            auto plain = std::make_shared<LayerNormalization>();
            plain->epsilon = fused->epsilon;
            nodes.absorb(st, (size_t)ln, out_name);
            st.in.push_back(id_of(lnn.inputs.at(1)));
            st.in.push_back(lnn.inputs.size() > 2 ? id_of(lnn.inputs[2]) : -1);
            st.kind_name = "Add+LayerNormalization";
            st.run = [fused, plain](Context &c, const InputList &in) {
                if (require(in, 0).shape() == require(in, 1).shape()) return fused->run(c, in);
                OutputList sum = Add().run(c, {in[0], in[1]}); // broadcasting Add: separate kernels
                return plain->run(c, {&sum[0], in[2], in[3]});
            };
            return true;
        }
        // Add(residual) -> RMSNormalization / SimplifiedLayerNormalization(last axis) as one skip launch.  The sum usually has other readers (it is the
        // residual stream), so the step runs where the Add stood and produces both values; the scale must exist by then.
        {
            const size_t at = st.pos;
            const std::string sum = out_name;
            auto us = nodes.users.find(sum);
            long rn = add_rms_consumer(nodes.m, at);
            if (rn >= 0 && nodes.dead[(size_t)rn]) rn = -1;
            if (rn >= 0) {
                const onnx::Node &c = nodes[rn];
                auto op = std::make_shared<AddRMSNormalization>();
                op->epsilon = c.get_float("epsilon", 1e-5f);
                op->want_sum = nodes.graph_outs.count(sum) != 0 || us->second.size() > 1;
                nodes.dead[(size_t)rn] = true; // (not absorb(): the step keeps the Add's position, the other readers of the sum come before the normalisation node)
                fused_away_++;
                out_name = c.outputs.at(0);
                st.in.push_back(id_of(c.inputs[1]));
                if (op->want_sum) st.extra_out = id_of(sum);
                st.kind_name = "Add+" + c.op_type;
                run_plainly(st, op);
                return true;
            }
        }
        const long sm = nodes.sole_user(out_name, "Softmax");
        if (sm >= 0 && nodes[sm].get_int("axis", -1) == -1) {
            // Add -> Softmax(last axis) = AddSoftmax (src/ops/attention.rs:94-156)
            nodes.absorb(st, (size_t)sm, out_name);
            st.kind_name = "AddSoftmax";
            st.run = [](Context &c, const InputList &in) {
                const Tensor &a = require(in, 0), &b = require(in, 1);
                AddSoftmax fused;
                const Tensor &x = a.len() >= b.len() ? a : b, &addend = a.len() >= b.len() ? b : a;
                auto unfused = [&] { OutputList sum = Add().run(c, in); return Softmax().run(c, {&sum[0]}); };
                // an addend of higher rank gives the sum that rank -- [R, C] + [1, 1, C] is [1, R, C] -- which the fused kernel's output, shaped like x, is not
                if (addend.ndim() > x.ndim()) return unfused();
                try {
                    return fused.run(c, {&x, &addend});
                } catch (const OpError &e) { // a broadcast the fused kernel does not cover: Add, then Softmax
                    if (e.kind != OpError::IncompatibleInputShapes) throw;
                    return unfused();
                }
            };
            return true;
        }
        return false;
    }
    // RMSNormalization / SimplifiedLayerNormalization, the skip forms and the two RotaryEmbedding operators: the read_decoder_node checks at load, one
    // launch per step, nothing read back (a position offset on the device is read by the kernel), so every one of them captures.  Rows of the batch are
    // independent unless a normalisation's axis resolves to dim 0; a skip form with a [1, S, H] or [S, H] skip reads the same skip rows for every batch row.
    void make_decoder_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        const DecoderNode a = read_decoder_node(m, n, st.name);
        const std::string nm = st.name;
        if (a.rotary) {
            if (a.contrib) {
                auto op = std::make_shared<RotaryEmbeddingMicrosoft>();
                op->interleaved = a.interleaved; op->num_heads = a.num_heads; op->rotary_embedding_dim = a.rotary_embedding_dim;
                st.kind_name = "com.microsoft.RotaryEmbedding";
                run_plainly(st, op);
            } else {
                auto op = std::make_shared<RotaryEmbedding>();
                op->interleaved = a.interleaved; op->num_heads = a.num_heads; op->rotary_embedding_dim = a.rotary_embedding_dim;
                run_plainly(st, op);
            }
        } else if (a.skip) {
            std::shared_ptr<SkipNormBase> op;
            if (a.rms) op = std::make_shared<SkipSimplifiedLayerNormalization>(); else op = std::make_shared<SkipLayerNormalization>();
            op->epsilon = *a.epsilon;
            op->want_sum = a.want_sum;
            st.run = [op](Context &c, const InputList &in) {
                OutputList o = op->run(c, in);
                while (o.size() < 4) o.emplace_back(); // outputs the graph names but nothing reads
                return o;
            };
        } else {
            std::shared_ptr<RMSNormalization> op;
            if (n.op_type == "RMSNormalization") op = std::make_shared<RMSNormalization>(); else op = std::make_shared<SimplifiedLayerNormalization>();
            op->axis = a.axis;
            op->epsilon = a.epsilon;
            st.batch_coupled = a.axis == 0;
            const std::string kind = n.op_type;
            st.run = [this, op, kind, nm](Context &c, const InputList &in) { note_axis(kind, nm, op->axis, require(in, 0)); return op->run(c, in); };
        }
    }
    // com.microsoft GroupQueryAttention: the read_gqa_node checks at load, then rten_hip_gqa_f32 per run.  seqlens_k and total_sequence_length stay on the
    // device and nothing is read back, so the step captures and a replayed plan follows new lengths; every batch item attends to its own cache only, so
    // the step is not batch_coupled.  The present outputs are handed on only when the graph reads them.
    void make_gqa_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        const GqaNode a = read_gqa_node(m, n, st.name);
        auto op = std::make_shared<GroupQueryAttention>();
        op->num_heads = a.num_heads; op->kv_num_heads = a.kv_num_heads; op->scale = a.scale;
        op->do_rotary = a.do_rotary; op->rotary_interleaved = a.rotary_interleaved; op->local_window_size = a.local_window_size;
        op->want_present = a.want_present;
        st.kind_name = "com.microsoft.GroupQueryAttention";
        const size_t named = n.outputs.size();
        st.run = [op, named](Context &c, const InputList &in) {
            OutputList o = op->run(c, in);
            while (o.size() < named) o.emplace_back(); // outputs the graph names but nothing reads
            return o;
        };
    }
    void make_activation_step(Step &st, const onnx::Node &n) {
        Activation act;
        if (activation_of(n, act)) { // parameters fixed at load time: one rten_hip_activation_f32 launch, nothing read back per run
            st.in.resize(1);
            run_plainly(st, std::make_shared<ActivationOp>(act.kind, act.alpha, act.beta));
        } else run_plainly(st, std::make_shared<Clip>()); // Clip with run-time bounds
    }
    void make_pool_step(Step &st, const onnx::Node &n) {
        std::vector<int> k = n.get_ints("kernel_shape", {});
        if (k.size() != 2) throw GraphError(n.op_type + " " + st.name + ": kernel_shape must have 2 values");
        const std::vector<int> strides = n.get_ints("strides", {1, 1});
        const Padding pad = padding_of(n, n.op_type.c_str());
        const bool ceil = n.get_int("ceil_mode", 0) != 0;
        if (n.outputs.size() > 1 && !n.outputs[1].empty()) throw GraphError("MaxPool " + st.name + ": the Indices output is not supported");
        auto finish = [&](auto op) { op->kernel_size = k; op->strides = strides; op->padding = pad; op->ceil_mode = ceil; run_plainly(st, op); return op; };
        if (n.op_type == "MaxPool") st.maxpool = finish(std::make_shared<MaxPool>());
        else finish(std::make_shared<AveragePool>())->count_include_pad = n.get_int("count_include_pad", 0) != 0;
    }
    // ReduceSum / ReduceMean; ReduceMax / ReduceMin and the int32 forms of ReduceL1 / ReduceSumSquare / ReduceProd (which shape arithmetic sometimes applies to a
    // shape vector: those run on the host); ReduceL2 / ReduceLogSum / ReduceLogSumExp.  Coupled to the batch exactly when dim 0 is reduced (read_reduce_attrs).
    void make_reduce_step(Step &st, const onnx::Node &n) {
        const std::string kind = n.op_type, nm = st.name;
        std::shared_ptr<ReduceOp> op;
        std::function<HostVal(const HostVal &, const std::vector<int> &)> host; // how a host value is reduced on the host, for the kinds shape arithmetic uses
        bool host_floats = false;                                               // ... float values too, not only int32 ones
        if (kind == "ReduceSum" || kind == "ReduceMean") {
            auto o = std::make_shared<ReduceSum>();
            o->mean = kind == "ReduceMean";
            op = o;
        } else if (const int rk = reduce_family_kind(kind); rk >= 0) {
            std::shared_ptr<Reduce> o;
            switch (rk) {
            case RTEN_HIP_REDUCE_L1: o = std::make_shared<ReduceL1>(); break;
            case RTEN_HIP_REDUCE_SUM_SQUARE: o = std::make_shared<ReduceSumSquare>(); break;
            case RTEN_HIP_REDUCE_L2: o = std::make_shared<ReduceL2>(); break;
            case RTEN_HIP_REDUCE_LOG_SUM: o = std::make_shared<ReduceLogSum>(); break;
            case RTEN_HIP_REDUCE_LOG_SUM_EXP: o = std::make_shared<ReduceLogSumExp>(); break;
            default: o = std::make_shared<ReduceProd>(); break;
            }
            if (o->int32) host = [o, rk](const HostVal &x, const std::vector<int> &ax) { return hostops::reduce_i32(x, ax, o->keep_dims, rk); }; // ReduceProd of a Shape
            op = o;
        } else {
            auto o = std::make_shared<ReduceMax>();
            o->min = kind == "ReduceMin";
            host = [o](const HostVal &x, const std::vector<int> &ax) { return hostops::reduce_minmax(x, ax, o->keep_dims, o->min); };
            host_floats = true;
            op = o;
        }
        read_reduce_attrs(st, n, *op);
        auto cache = std::make_shared<HostCache>();
        st.run = [this, op, kind, nm, host, host_floats, cache](Context &c, const InputList &in) {
            const Tensor &x = require(in, 0);
            for (int a : op->axes) note_axis(kind, nm, a, x);
            // shape arithmetic stays on the host -- but not a 0-d value and not the no-op form, which are the operator's
            if (host && x.host() && (host_floats || !x.host()->is_float) && x.ndim() > 0 && !(op->axes.empty() && op->noop_with_empty_axes)) {
                OutputList o;
                o.push_back(materialize(c, host(*x.host(), resolve_axes(op->axes, x.ndim())), *cache));
                return o;
            }
            return op->run(c, in);
        };
    }
    // InstanceNormalization / BatchNormalization (+ Relu, or one activation activation_of takes: the activation sees the f32 value the unfused node would
    // store, so the pair keeps its bits) and LogSoftmax.  BatchNormalization is NOT folded into a preceding Conv: that would change bits against the
    // reference.  Rows of the batch are independent for the two normalisations; LogSoftmax is coupled exactly when its axis resolves to dim 0.
    void make_norm_step(Step &st, const onnx::Node &n, Nodes &nodes, std::string &out_name) {
        const NormNode a = read_norm_node(n, st.name);
        const std::string kind = n.op_type, nm = st.name;
        if (kind == "LogSoftmax") {
            auto op = std::make_shared<LogSoftmax>();
            op->axis = a.axis;
            st.batch_coupled = op->axis == 0;
            st.run = [this, op, nm](Context &c, const InputList &in) { note_axis("LogSoftmax", nm, op->axis, require(in, 0)); return op->run(c, in); };
            return;
        }
        Activation act;
        if (opt_.fuse) {
            const long r = nodes.sole_user(out_name, "Relu");
            if (r >= 0) { act.kind = RTEN_HIP_ACT_RELU; nodes.absorb(st, (size_t)r, out_name); }
            else {
                Activation follower;
                const long ac = nodes.sole_activation(out_name, follower);
                if (ac >= 0) { act = follower; nodes.absorb(st, (size_t)ac, out_name); }
            }
        }
        if (act.kind != RTEN_HIP_ACT_NONE) st.kind_name = kind + "+" + activation_name(act.kind);
        if (kind == "InstanceNormalization") {
            auto op = std::make_shared<InstanceNormalization>();
            op->epsilon = a.epsilon;
            op->act = act;
            run_plainly(st, op);
        } else {
            auto op = std::make_shared<BatchNormalization>();
            op->epsilon = a.epsilon.value_or(1e-5f);
            op->act = act;
            run_plainly(st, op);
        }
    }

    // Neg / Abs / Sign / Floor / Ceil / Round / Sqrt / Reciprocal / Min / Max: on the host when every operand is a host value (shape arithmetic: exporters
    // write F.interpolate(scale_factor=..) as Shape -> Cast -> Mul -> Floor -> Cast, attention scaling as Sqrt(Cast(Shape[-1]))), on the device otherwise.
    // Exp / Log / Softplus / Pow / PRelu / Sum / Mean run on the device always: a host value's device copy is the operand and the result carries no host value.
    void make_math_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        const std::string kind = n.op_type;
        if (kind == "Pow") check_pow_node(m, n, st.name);
        static const OpRegistry reg = OpRegistry::with_all_ops();
        std::shared_ptr<Operator> op(reg.create(kind).release());
        if (!is_hostable_math_kind(kind)) { run_plainly(st, op); return; }
        if (kind == "Min" || kind == "Max")
            make_hostable(st, [kind](const std::vector<const HostVal *> &v, HostVal &out) { return hostops::minmax_fold(kind == "Min", v, out); },
                          [op](Context &c, const InputList &in) { return op->run(c, in); });
        else
            make_hostable(st, [kind](const std::vector<const HostVal *> &v, HostVal &out) { return v.size() == 1 && v[0] && hostops::unary(kind, *v[0], out); },
                          [op](Context &c, const InputList &in) { return op->run(c, in); });
    }

    // Pad: read_pad_node's checks at load; before opset 11 the pads / value attributes, otherwise pads and constant_value are host values at run time
    // (constants or shape arithmetic), read as Slice reads its starts: nothing is read back, the step is one rten_hip_pad_b32 launch and capture-safe.  A
    // host-valued operand in constant mode is padded on the host (exporters pad shape vectors).  A pad or crop of dim 0 couples the batch rows (sub-batch
    // chains split dim 0).
    void make_pad_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        const std::string nm = st.name;
        const PadNode a = read_pad_node(m, n, nm);
        auto cache = std::make_shared<HostCache>();
        st.run = [this, nm, a, cache](Context &c, const InputList &in) {
            const Tensor &x = require(in, 0);
            const std::vector<int64_t> pads = a.attr_form ? a.pads : host_ints(&require(in, 1), "Pad: pads");
            const Tensor *value = a.attr_form ? nullptr : get(in, 2);
            if (value && !value->host()) throw OpError(OpError::UnsupportedValue, "Pad: constant_value must be a constant or computable from the input shapes (it depends on device data)");
            const size_t nd = (size_t)x.ndim();
            if (nd > 0 && pads.size() == 2 * nd && (pads[0] != 0 || pads[nd] != 0) && runtime_coupled_.empty()) runtime_coupled_ = "Pad \"" + nm + "\" (pads or crops dim 0)";
            OutputList o;
            if (x.host() && a.mode == RTEN_HIP_PAD_CONSTANT) {
                HostVal attr_fill, out;
                attr_fill.is_float = x.host()->is_float;
                if (attr_fill.is_float) attr_fill.f = {a.value}; else attr_fill.i = {(int64_t)a.value};
                if (hostops::pad_constant(*x.host(), pads, a.attr_form ? &attr_fill : (value ? value->host() : nullptr), out)) { o.push_back(materialize(c, std::move(out), *cache)); return o; }
            }
            uint32_t fill_bits = 0;
            if (!a.attr_form) fill_bits = Pad::fill_word(x, value);
            else if (x.dtype() == DType::F32) std::memcpy(&fill_bits, &a.value, 4);
            else fill_bits = (uint32_t)(int32_t)a.value;
            o.push_back(pad_tensor(c, x, pads, a.mode, fill_bits));
            return o;
        };
    }

    // NonMaxSuppression: read_nms_node's checks at load.  The three scalar operands are host values at run time (the operator refuses a device-valued one that
    // is not a graph input).  One selected list serves every image, so the step is batch_coupled: no sub-batch chains.  It READS BACK the row count to shape
    // its output -- the one kind of step that does: it synchronises the stream once per run, capture() refuses the plan before it begins (reads_back), and
    // what follows it (Gather of the boxes by selected[:, 2], Slice, Squeeze) sees an ordinary run-time shape.
    void make_nms_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        auto op = std::make_shared<NonMaxSuppression>();
        op->center_point_box = read_nms_node(m, n, st.name).center_point_box;
        st.batch_coupled = true;
        st.reads_back = true;
        run_plainly(st, op);
    }

    // DFT / STFT: read_dft_node's / read_stft_node's checks at load.  dft_length, axis, frame_step and frame_length are host values at run time (constants or
    // shape arithmetic), read as Pad reads its pads; the window is a constant or a device tensor.  Nothing is read back: a step is the twiddle prologue and one
    // launch of rten_amd/csrc/fft.hip (plus two transposes for a DFT axis other than ndim - 2) and captures.  A DFT whose axis resolves to dim 0 couples the
    // batch rows (sub-batch chains split dim 0); STFT transforms within a row and never does.
    void make_fft_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        const std::string nm = st.name;
        auto one_int = [](const Tensor &t, const std::string &what) {
            if (t.dtype() != DType::I32) throw OpError(OpError::InputCastFailed, "expected int32 tensor");
            const std::vector<int64_t> v = host_ints(&t, what);
            if (v.size() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
            return v[0];
        };
        if (n.op_type == "DFT") {
            const DftNode a = read_dft_node(m, n, nm);
            st.batch_coupled = a.axis_fixed && a.axis == 0; // (a negative axis that resolves to dim 0, or an axis input, is a run-time fact: below)
            st.run = [this, a, nm, one_int](Context &c, const InputList &in) {
                const Tensor &x = require(in, 0);
                const Tensor *len = get(in, 1), *ax = a.axis_fixed ? nullptr : get(in, 2);
                const int64_t dft_length = len ? one_int(*len, "DFT: dft_length") : 0;
                const int64_t axis = a.axis_fixed ? a.axis : (ax ? one_int(*ax, "DFT: axis") : -2);
                if (x.ndim() > 0 && (axis == 0 || axis + x.ndim() == 0) && runtime_coupled_.empty()) runtime_coupled_ = "DFT \"" + nm + "\" (transforms along dim 0)";
                OutputList o;
                o.push_back(dft_tensor(c, x, len != nullptr, dft_length, axis, a.inverse, a.onesided));
                return o;
            };
        } else {
            const StftNode a = read_stft_node(m, n, nm);
            st.run = [a, one_int](Context &c, const InputList &in) {
                const Tensor &signal = require(in, 0);
                const int64_t frame_step = one_int(require(in, 1), "STFT: frame_step");
                const Tensor *fl = get(in, 3);
                const int64_t frame_length = fl ? one_int(*fl, "STFT: frame_length") : 0;
                OutputList o;
                o.push_back(stft_tensor(c, signal, frame_step, get(in, 2), fl != nullptr, frame_length, a.onesided));
                return o;
            };
        }
    }

    // CumSum / GatherElements / Trilu / Tile: the read_*_node checks at load.  CumSum's axis, Trilu's k and Tile's repeats are host values at run time (constants
    // or shape arithmetic), read as Slice reads its starts: nothing is read back, each step is one launch of rten_amd/csrc/scan.hip and capture-safe.  When the
    // data operand (and GatherElements' indices) are host values too, the step is evaluated on the host (hostops::cumsum / gather_elements / trilu / tile): an
    // exporter's triu(full((S, S))) mask or the repeat of a shape vector costs no launch.  A host-valued data operand with device indices (RoBERTa's buffered
    // token_type_ids) runs on the data's cached device copy.  On the device path the rows of dim 0 are coupled (sub-batch chains split dim 0) when CumSum or
    // GatherElements resolve to axis 0, when repeats[0] != 1, and when Trilu runs on a rank-2 operand (dim 0 is its row index); a host-evaluated value is
    // not split.
    void make_index_step(Step &st, const onnx::Node &n, const onnx::Model &m) {
        const std::string kind = n.op_type, nm = st.name;
        auto couple = [this, kind, nm](const char *why) { if (runtime_coupled_.empty()) runtime_coupled_ = kind + " \"" + nm + "\" (" + why + ")"; };
        auto one_int = [kind](const Tensor &t, const char *what) {
            const std::vector<int64_t> v = host_ints(&t, kind + ": " + what);
            if (v.size() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
            return v[0];
        };
        if (kind == "CumSum") {
            const CumSumNode a = read_cumsum_node(m, n, nm);
            if (const onnx::TensorProto *t = initializer_named(m, n.inputs[1])) { // a constant axis 0 is known at load; a negative one resolves at run time
                int64_t v = -1;
                if (t->data_type == onnx::INT64 && t->raw.size() == 8) std::memcpy(&v, t->raw.data(), 8);
                else if (t->data_type == onnx::INT32 && t->raw.size() == 4) { int32_t w; std::memcpy(&w, t->raw.data(), 4); v = w; }
                st.batch_coupled = v == 0;
            }
            make_hostable(st,
                          [a](const std::vector<const HostVal *> &v, HostVal &out) {
                              if (v.size() != 2 || !v[0] || !v[1] || v[1]->is_float || v[1]->i.size() != 1) return false;
                              out = hostops::cumsum(*v[0], v[1]->i[0], a.exclusive, a.reverse);
                              return true;
                          },
                          [a, couple, one_int](Context &c, const InputList &in) {
                              const Tensor &x = require(in, 0);
                              const int64_t axis = one_int(require(in, 1), "axis");
                              if (x.ndim() > 0 && (axis == 0 || axis + x.ndim() == 0)) couple("sums along dim 0");
                              OutputList o;
                              o.push_back(cumsum_tensor(c, x, axis, a.exclusive, a.reverse));
                              return o;
                          });
        } else if (kind == "GatherElements") {
            const int axis = read_gather_elements_node(n, nm).axis;
            st.batch_coupled = axis == 0;
            make_hostable(st,
                          [axis](const std::vector<const HostVal *> &v, HostVal &out) {
                              if (v.size() != 2 || !v[0] || !v[1] || v[1]->is_float) return false;
                              out = hostops::gather_elements(*v[0], *v[1], axis);
                              return true;
                          },
                          [this, axis, nm](Context &c, const InputList &in) {
                              note_axis("GatherElements", nm, axis, require(in, 0));
                              OutputList o;
                              o.push_back(gather_elements_tensor(c, require(in, 0), require(in, 1), axis));
                              return o;
                          });
        } else if (kind == "Trilu") {
            const bool upper = read_trilu_node(m, n, nm).upper;
            make_hostable(st,
                          [upper](const std::vector<const HostVal *> &v, HostVal &out) {
                              if (v.empty() || v.size() > 2 || !v[0]) return false;
                              if (v.size() == 2 && v[1] && (v[1]->is_float || v[1]->i.size() != 1)) return false;
                              out = hostops::trilu(*v[0], v.size() == 2 && v[1] ? v[1]->i[0] : 0, upper);
                              return true;
                          },
                          [upper, couple, one_int](Context &c, const InputList &in) {
                              const Tensor &x = require(in, 0);
                              const int64_t k = get(in, 1) ? one_int(*get(in, 1), "k") : 0;
                              if (x.ndim() == 2) couple("dim 0 is the matrix row");
                              OutputList o;
                              o.push_back(trilu_tensor(c, x, k, upper));
                              return o;
                          });
        } else {
            read_tile_node(m, n, nm);
            make_hostable(st,
                          [](const std::vector<const HostVal *> &v, HostVal &out) {
                              if (v.size() != 2 || !v[0] || !v[1] || v[1]->is_float || v[1]->shape.size() != 1) return false;
                              return hostops::tile(*v[0], v[1]->i, out);
                          },
                          [couple](Context &c, const InputList &in) {
                              const Tensor &x = require(in, 0), &r = require(in, 1);
                              const std::vector<int64_t> repeats = host_ints(&r, "Tile: repeats");
                              if (r.ndim() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 1 dims");
                              if (!repeats.empty() && repeats[0] != 1) couple("repeats dim 0");
                              OutputList o;
                              o.push_back(tile_tensor(c, x, repeats));
                              return o;
                          });
        }
    }

    // QuantizeLinear / DequantizeLinear: read_qdq_node's checks at load.  With fusion on, a QuantizeLinear whose value only feeds a DequantizeLinear with the same
    // constant parameters (qdq_pair_partner) becomes one round-trip step on rten_hip_quantize_dequantize_f32; otherwise each node is its own step.  Scales and
    // zero points stay device operands (they may be run-time values): nothing is read back, the steps are capture-safe.  A per-axis step whose axis resolves to
    // dim 0 couples the batch rows.  (A DequantizeLinear over initializers never gets here: canonicalize folded it.)
    void make_qdq_step(Step &st, const onnx::Node &n, const onnx::Model &m, Nodes &nodes, std::string &out_name) {
        const std::string nm = st.name, kind = n.op_type;
        const QdqNode a = read_qdq_node(m, n, nm);
        const int axis = a.axis;
        if (const onnx::TensorProto *sc = n.inputs.size() > 1 ? initializer_named(m, n.inputs[1]) : nullptr) st.batch_coupled = sc->len() != 1 && axis == 0;
        auto note = [this, nm, kind, axis](const InputList &in) { if (require(in, 1).len() != 1) note_axis(kind, nm, axis, require(in, 0)); };
        if (!a.quantize) {
            auto op = std::make_shared<DequantizeLinear>();
            op->axis = axis;
            st.run = [op, note](Context &c, const InputList &in) { note(in); return op->run(c, in); };
            return;
        }
        const long partner = opt_.fuse ? qdq_pair_partner(m, st.pos) : -1;
        if (partner >= 0 && !nodes.dead[(size_t)partner]) {
            read_qdq_node(m, nodes[partner], label_of(nodes[partner]));
            auto op = std::make_shared<QuantizeDequantizeLinear>();
            op->q.axis = axis;
            op->q.output_dtype = a.output_dtype;
            nodes.absorb(st, (size_t)partner, out_name);
            st.kind_name = "QuantizeLinear+DequantizeLinear";
            st.run = [op, note](Context &c, const InputList &in) { note(in); return op->run(c, in); };
            return;
        }
        auto op = std::make_shared<QuantizeLinear>();
        op->axis = axis;
        op->output_dtype = a.output_dtype;
        st.run = [op, note](Context &c, const InputList &in) { note(in); return op->run(c, in); };
    }

    // ArgMax / ArgMin, TopK and Softmax: one axis each, noted per run in case it resolves to dim 0
    void make_select_step(Step &st, const onnx::Node &n) {
        const std::string kind = n.op_type, nm = st.name;
        if (kind == "ArgMax" || kind == "ArgMin") {
            if (n.get_int("select_last_index", 0) != 0) throw GraphError(kind + " " + st.name + ": select_last_index is not supported"); // onnx_registry.rs:769
            auto op = std::make_shared<ArgMax>();
            op->min = kind == "ArgMin";
            op->axis = (int)n.get_int("axis", 0);
            op->keep_dims = n.get_int("keepdims", 1) != 0;
            st.batch_coupled = op->axis == 0;
            st.run = [this, op, kind, nm](Context &c, const InputList &in) { note_axis(kind, nm, op->axis, require(in, 0)); return op->run(c, in); };
        } else if (kind == "TopK") {
            auto op = std::make_shared<TopK>();
            op->axis = (int)n.get_int("axis", -1);
            op->largest = n.get_int("largest", 1) != 0;
            op->sorted = n.get_int("sorted", 1) != 0;
            if (n.inputs.size() < 2 || n.inputs[1].empty()) throw GraphError("TopK " + st.name + ": the K input is missing");
            // K is read on the host (no read-back, so the step may be captured): an initializer, a Constant, or shape arithmetic the executor evaluates
            // on the host.  A graph input is device data at run time: refused here; any other device-computed K is refused by the step when it runs.
            for (auto &gi : inputs_)
                if (gi.name == n.inputs[1] && !is_const(gi.name))
                    throw GraphError("TopK " + st.name + ": K must be a constant or computable from the input shapes (it is the graph input \"" + gi.name + "\", device data at run time)");
            st.batch_coupled = op->axis == 0;
            st.run = [this, op, nm](Context &c, const InputList &in) {
                note_axis("TopK", nm, op->axis, require(in, 0));
                host_ints(&require(in, 1), "TopK: K"); // throws unless K carries a host value
                return op->run(c, in);
            };
        } else {
            auto op = std::make_shared<Softmax>();
            op->axis = (int)n.get_int("axis", -1);
            st.batch_coupled = op->axis == 0;
            st.run = [this, op, nm](Context &c, const InputList &in) { note_axis("Softmax", nm, op->axis, require(in, 0)); return op->run(c, in); };
        }
    }

    // Layout / logic operators around the hot path (src/ops/layout.rs, slice.rs, concat.rs, gather.rs, convert.rs, binary_elementwise.rs, non_zero.rs,
    // generate.rs): each runs on the host when its operands are host values and as a device kernel otherwise.  Returns false for other operator types.
    bool make_layout_step(Step &st, const onnx::Node &n) {
        const std::string op = n.op_type, name = st.name;
        static const std::map<std::string, int> ew = {{"And", RTEN_HIP_EW_AND}, {"Or", RTEN_HIP_EW_OR}, {"Xor", RTEN_HIP_EW_XOR}, {"Equal", RTEN_HIP_EW_EQUAL},
                                                      {"Less", RTEN_HIP_EW_LESS}, {"LessOrEqual", RTEN_HIP_EW_LESS_EQ}, {"Greater", RTEN_HIP_EW_GREATER},
                                                      {"GreaterOrEqual", RTEN_HIP_EW_GREATER_EQ}};
        static const std::map<std::string, int> arith = {{"Add", RTEN_HIP_EW_IADD}, {"Sub", RTEN_HIP_EW_ISUB}, {"Mul", RTEN_HIP_EW_IMUL}, {"Div", RTEN_HIP_EW_IDIV}};
        if (op == "Shape") { // src/ops/layout.rs:475-520 (start / end attributes of opset 15)
            const int64_t start = n.get_int("start", 0);
            const bool has_end = n.attr("end") != nullptr;
            const int64_t end = n.get_int("end", 0);
            auto cache = std::make_shared<HostCache>();
            st.run = [start, has_end, end, cache](Context &c, const InputList &in) {
                const Tensor &x = require(in, 0);
                OutputList o;
                o.push_back(materialize(c, hostops::shape_of(x.shape(), start, has_end, end), *cache));
                return o;
            };
            return true;
        }
        if (ew.count(op) || arith.count(op)) {
            const bool is_arith = arith.count(op) != 0;
            const int code = is_arith ? arith.at(op) : ew.at(op);
            std::shared_ptr<Operator> fop;
            if (is_arith) { static const OpRegistry reg = OpRegistry::with_all_ops(); fop.reset(reg.create(op).release()); }
            auto dev = std::make_shared<ElementwiseNd>(code, is_arith ? "IntegerArithmetic" : "Logical");
            make_hostable(st,
                          [op](const std::vector<const HostVal *> &v, HostVal &out) { return v.size() == 2 && v[0] && v[1] && hostops::binary(op, *v[0], *v[1], out); },
                          [dev, fop, is_arith](Context &c, const InputList &in) {
                              if (is_arith && !(require(in, 0).dtype() == DType::I32 && require(in, 1).dtype() == DType::I32)) return fop->run(c, in); // the f32 kernels
                              if (is_arith && dev->code == RTEN_HIP_EW_IDIV && in[1]->host())
                                  for (int64_t d : in[1]->host()->i) if (d == 0) throw OpError(OpError::InvalidValue, "Divisor contains zero");
                              return dev->run(c, in);
                          });
            return true;
        }
        if (op == "Not") {
            auto dev = std::make_shared<ElementwiseNd>(RTEN_HIP_EW_NOT, "Not");
            make_hostable(st,
                          [](const std::vector<const HostVal *> &v, HostVal &out) { return v.size() == 1 && v[0] && hostops::logical_not(*v[0], out); },
                          [dev](Context &c, const InputList &in) { return dev->run(c, in); });
            return true;
        }
        if (op == "Where") {
            auto dev = std::make_shared<Where>();
            make_hostable(st, [](const std::vector<const HostVal *> &v, HostVal &out) { return v.size() == 3 && v[0] && v[1] && v[2] && hostops::where(*v[0], *v[1], *v[2], out); },
                          [dev](Context &c, const InputList &in) { return dev->run(c, in); });
            return true;
        }
        if (op == "Cast") {
            auto dev = std::make_shared<Cast>();
            dev->to = dtype_of((int)n.get_int("to", onnx::FLOAT), name);
            const DType to = dev->to;
            make_hostable(st, [to](const std::vector<const HostVal *> &v, HostVal &out) { if (v.size() != 1 || !v[0] || (to != DType::F32 && to != DType::I32)) return false; out = hostops::cast(*v[0], to); return true; },
                          [dev](Context &c, const InputList &in) { return dev->run(c, in); });
            return true;
        }
        if (op == "Transpose") {
            auto dev = std::make_shared<Transpose>();
            dev->perm = n.get_ints("perm", {});
            const std::vector<int> perm = dev->perm;
            make_hostable(st, [perm](const std::vector<const HostVal *> &v, HostVal &out) { if (v.size() != 1 || !v[0]) return false; out = hostops::transpose(*v[0], perm); return true; },
                          [this, dev, name](Context &c, const InputList &in) {
                              const int nd = require(in, 0).ndim(); // a device transpose that moves dim 0 mixes the rows sub-batch chains would split
                              const int p0 = dev->perm.empty() ? nd - 1 : (dev->perm[0] < 0 ? dev->perm[0] + nd : dev->perm[0]);
                              if (nd > 1 && p0 != 0 && runtime_coupled_.empty()) runtime_coupled_ = "Transpose \"" + name + "\" (moves dim 0)";
                              return dev->run(c, in);
                          });
            return true;
        }
        if (op == "Gather") {
            auto dev = std::make_shared<Gather>();
            dev->axis = (int)n.get_int("axis", 0);
            const int axis = dev->axis;
            make_hostable(st, [axis](const std::vector<const HostVal *> &v, HostVal &out) { if (v.size() != 2 || !v[0] || !v[1] || v[1]->is_float) return false; out = hostops::gather(*v[0], *v[1], axis); return true; },
                          [dev](Context &c, const InputList &in) { return dev->run(c, in); });
            return true;
        }
        if (op == "Concat") {
            if (!n.attr("axis")) throw GraphError("Concat " + name + ": the axis attribute is missing");
            const int axis = (int)n.get_int("axis", 0);
            make_hostable(st,
                          [axis](const std::vector<const HostVal *> &v, HostVal &out) { for (auto *x : v) if (!x) return false; if (v.empty()) return false; out = hostops::concat(v, axis); return true; },
                          [axis](Context &c, const InputList &in) { OutputList o; o.push_back(concat_tensors(c, in, axis)); return o; });
            return true;
        }
        if (op == "Slice") { // opset >= 10: starts, ends, axes, steps as inputs (host values); opset 1: attributes
            std::vector<int64_t> a_starts, a_ends, a_axes;
            if (const onnx::Attr *a = n.attr("starts")) a_starts = a->ints;
            if (const onnx::Attr *a = n.attr("ends")) a_ends = a->ints;
            if (const onnx::Attr *a = n.attr("axes")) a_axes = a->ints;
            const bool attr_form = n.attr("starts") != nullptr;
            auto cache = std::make_shared<HostCache>();
            st.run = [attr_form, a_starts, a_ends, a_axes, cache](Context &c, const InputList &in) {
                const Tensor &x = require(in, 0);
                const std::vector<int64_t> starts = attr_form ? a_starts : host_ints(in.size() > 1 ? in[1] : nullptr, "Slice: starts"),
                                           ends = attr_form ? a_ends : host_ints(in.size() > 2 ? in[2] : nullptr, "Slice: ends"),
                                           axes = attr_form ? a_axes : host_ints(in.size() > 3 ? in[3] : nullptr, "Slice: axes"),
                                           steps = attr_form ? std::vector<int64_t>{} : host_ints(in.size() > 4 ? in[4] : nullptr, "Slice: steps");
                const std::vector<SliceRange> r = resolve_slice(x.shape(), starts, ends, axes, steps);
                OutputList o;
                if (x.host()) o.push_back(materialize(c, hostops::slice(*x.host(), r), *cache));
                else o.push_back(slice_tensor(c, x, r));
                return o;
            };
            return true;
        }
        if (op == "Expand") {
            auto cache = std::make_shared<HostCache>();
            st.run = [cache](Context &c, const InputList &in) {
                const Tensor &x = require(in, 0);
                const std::vector<int64_t> target = host_ints(&require(in, 1), "Expand: the shape input");
                hostops::check_expand(x.shape(), target);
                OutputList o;
                if (x.host() && detail::prod(target, 0, target.size()) <= hostops::kMaxHostElems) o.push_back(materialize(c, hostops::expand(*x.host(), target), *cache));
                else o.push_back(expand_to(c, x, target));
                return o;
            };
            return true;
        }
        if (op == "ConstantOfShape") { // src/ops/generate.rs: a tensor of `shape` filled with the `value` attribute (default float 0)
            HostVal fill;
            fill.is_float = true; fill.f = {0.f};
            if (const onnx::Attr *v = n.attr("value")) {
                const onnx::TensorProto &t = v->t;
                if (t.len() != 1) throw GraphError("ConstantOfShape " + name + ": value must hold one element");
                if (t.data_type == onnx::FLOAT && t.raw.size() == 4) std::memcpy(&fill.f[0], t.raw.data(), 4);
                else if (t.data_type == onnx::INT64 && t.raw.size() == 8) { int64_t x; std::memcpy(&x, t.raw.data(), 8); fill.is_float = false; fill.f.clear(); fill.i = {hostops::saturate32(x)}; }
                else if (t.data_type == onnx::INT32 && t.raw.size() == 4) { int32_t x; std::memcpy(&x, t.raw.data(), 4); fill.is_float = false; fill.f.clear(); fill.i = {x}; }
                else if (t.data_type == onnx::BOOL && t.raw.size() == 1) { fill.is_float = false; fill.f.clear(); fill.i = {t.raw[0] != 0}; }
                else throw GraphError("ConstantOfShape " + name + ": unsupported value type");
            }
            auto cache = std::make_shared<HostCache>();
            st.run = [fill, cache](Context &c, const InputList &in) {
                const std::vector<int64_t> shape = host_ints(&require(in, 0), "ConstantOfShape: the shape input");
                OutputList o;
                if (detail::prod(shape, 0, shape.size()) <= hostops::kMaxHostElems) { o.push_back(materialize(c, hostops::constant_fill(fill, shape), *cache)); return o; }
                for (int64_t d : shape) if (d < 0) throw OpError(OpError::InvalidValue, "Invalid shape");
                Tensor one = materialize(c, HostVal(fill), *cache); // a large fill: expand the one-element device constant
                o.push_back(expand_to(c, one, shape));
                return o;
            };
            return true;
        }
        if (op == "NonZero") { // the output's shape depends on the input's VALUES: only host values (exporters write arange(n) as NonZero(ConstantOfShape(n)))
            auto cache = std::make_shared<HostCache>();
            st.run = [cache](Context &c, const InputList &in) {
                const Tensor &x = require(in, 0);
                if (!x.host()) throw OpError(OpError::UnsupportedValue, "NonZero of device data: the output shape would depend on values (only shape-derived operands are supported)");
                OutputList o;
                o.push_back(materialize(c, hostops::nonzero(*x.host()), *cache));
                return o;
            };
            return true;
        }
        if (op == "Range") { // src/ops/generate.rs: start, limit, delta scalars (host values)
            auto cache = std::make_shared<HostCache>();
            st.run = [cache](Context &c, const InputList &in) {
                const Tensor &a = require(in, 0), &b = require(in, 1), &d = require(in, 2);
                if (!a.host() || !b.host() || !d.host()) throw OpError(OpError::UnsupportedValue, "Range: start / limit / delta must be constants or computable from the input shapes");
                HostVal out = hostops::range(*a.host(), *b.host(), *d.host());
                OutputList o;
                o.push_back(materialize(c, std::move(out), *cache));
                return o;
            };
            return true;
        }
        return false;
    }

    // Resize (opset 10: [X, scales]; 11+: [X, roi, scales, sizes]) and Upsample (opset 7: the `scales` attribute; 9: input 1) with the attributes the
    // reference reads (onnx_registry.rs:1721-1810).  Scales / sizes are host values at run time (constants or shape arithmetic): nothing is read back,
    // and the step is one rten_hip_resize_f32 launch (a device copy when nothing is resized), so it is capture-safe.
    void make_resize_step(Step &st, const onnx::Node &n) {
        const std::string kind = n.op_type, name = st.name;
        std::shared_ptr<Resize> op = kind == "Upsample" ? std::make_shared<Upsample>() : std::make_shared<Resize>();
        auto str_attr = [&](const char *a, const std::string &dflt) { const onnx::Attr *at = n.attr(a); return at ? at->s : dflt; };
        const std::string mode = str_attr("mode", "nearest");
        if (mode == "nearest") op->mode = RTEN_HIP_RESIZE_MODE_NEAREST;
        else if (mode == "linear" || (kind == "Resize" && mode == "cubic")) op->mode = RTEN_HIP_RESIZE_MODE_LINEAR; // cubic: linear, as the reference does
        else throw GraphError(kind + " " + name + ": mode \"" + mode + "\" is not supported");
        size_t scales_at = 1; // the scales input (sizes follow it in opset 11+)
        if (kind == "Resize") {
            if (n.get_int("antialias", 0) != 0 || n.get_int("exclude_outside", 0) != 0 || n.get_float("extrapolation_value", 0.f) != 0.f ||
                n.get_float("cubic_coeff_a", -0.75f) != -0.75f || str_attr("keep_aspect_ratio_policy", "stretch") != "stretch")
                throw GraphError("Resize " + name + ": antialias, exclude_outside, extrapolation_value, cubic_coeff_a and keep_aspect_ratio_policy must keep their defaults");
            static const std::map<std::string, int32_t> coords = {{"half_pixel", RTEN_HIP_RESIZE_COORD_HALF_PIXEL}, {"asymmetric", RTEN_HIP_RESIZE_COORD_ASYMMETRIC},
                                                                  {"align_corners", RTEN_HIP_RESIZE_COORD_ALIGN_CORNERS},
                                                                  {"pytorch_half_pixel", RTEN_HIP_RESIZE_COORD_PYTORCH_HALF_PIXEL}};
            static const std::map<std::string, int32_t> nearest = {{"round_prefer_floor", RTEN_HIP_RESIZE_NEAREST_ROUND_PREFER_FLOOR},
                                                                   {"round_prefer_ceil", RTEN_HIP_RESIZE_NEAREST_ROUND_PREFER_CEIL},
                                                                   {"floor", RTEN_HIP_RESIZE_NEAREST_FLOOR}, {"ceil", RTEN_HIP_RESIZE_NEAREST_CEIL}};
            const std::string cm = str_attr("coordinate_transformation_mode", "half_pixel"), nm = str_attr("nearest_mode", "round_prefer_floor");
            if (!coords.count(cm)) throw GraphError("Resize " + name + ": coordinate_transformation_mode \"" + cm + "\" is not supported");
            if (!nearest.count(nm)) throw GraphError("Resize " + name + ": nearest_mode \"" + nm + "\" is not supported");
            op->coord_mode = coords.at(cm);
            op->nearest_mode = nearest.at(nm);
            if (n.inputs.size() == 2) { // the opset-10 form [X, scales], which PyTorch's exporter also writes under later opsets: Upsample's coordinates
                op->coord_mode = RTEN_HIP_RESIZE_COORD_ASYMMETRIC;
                op->nearest_mode = RTEN_HIP_RESIZE_NEAREST_FLOOR;
            } else scales_at = 2;
        }
        const onnx::Attr *sa = kind == "Upsample" ? n.attr("scales") : nullptr;
        const std::vector<float> attr_scales = sa ? sa->floats : std::vector<float>();
        if (sa) st.in.resize(1);
        // a constant scales / sizes operand of length 1 or 2 means a 1-D / 2-D input, whose dim 0 is resampled
        int64_t rank = sa ? (int64_t)attr_scales.size() : -1;
        for (size_t k = scales_at; !sa && rank < 0 && k < n.inputs.size() && k <= scales_at + 1; k++)
            if (is_const(n.inputs[k]) && const_of(n.inputs[k]).len() > 0) rank = const_of(n.inputs[k]).len();
        st.batch_coupled = rank == 1 || rank == 2;
        const bool two_input = scales_at == 1;
        st.run = [this, op, kind, name, sa_given = sa != nullptr, attr_scales, scales_at, two_input](Context &c, const InputList &in) {
            const Tensor &x = require(in, 0);
            ResizeTarget t;
            if (sa_given) t.s = attr_scales;
            else {
                const Tensor *s = get(in, scales_at), *z = two_input ? nullptr : get(in, scales_at + 1);
                for (const Tensor *v : {s, z})
                    if (v && v->len() && !v->host())
                        throw OpError(OpError::UnsupportedValue, kind + ": scales / sizes must be constants or computable from the input shapes (they depend on device data)");
                t = two_input ? Resize::scales_target(require(in, 1)) : Resize::target(s, z);
            }
            OutputList o;
            o.push_back(op->resize(c, x, t));
            if (x.ndim() <= 2 && o[0].shape() != x.shape() && runtime_coupled_.empty()) runtime_coupled_ = kind + " \"" + name + "\" (resizes dim 0)";
            return o;
        };
    }

    // Split (onnx_registry.rs:1962-1972): the `split` attribute (opset < 13), the split input (13+) or `num_outputs` (18+), else the node's output count.
    // Host values split on the host (shape arithmetic); 4-byte device tensors are one strided copy per piece.
    void make_split_step(Step &st, const onnx::Node &n) {
        auto op = std::make_shared<Split>();
        op->axis = (int)n.get_int("axis", 0);
        op->num_outputs = n.attr("num_outputs") ? n.get_int("num_outputs", 0) : -1;
        op->node_outputs = (int64_t)n.outputs.size();
        const onnx::Attr *sa = n.attr("split");
        const std::vector<int64_t> attr_split = sa ? sa->ints : std::vector<int64_t>();
        if (sa) st.in.resize(1);
        st.batch_coupled = op->axis == 0;
        std::vector<std::shared_ptr<HostCache>> caches;
        for (size_t k = 0; k < n.outputs.size(); k++) caches.push_back(std::make_shared<HostCache>());
        const std::string name = st.name;
        st.run = [this, op, sa_given = sa != nullptr, attr_split, caches, name](Context &c, const InputList &in) {
            const Tensor &x = require(in, 0);
            note_axis("Split", name, op->axis, x);
            const int a = resolve_axis(op->axis, x.ndim());
            const Tensor *s = sa_given ? nullptr : get(in, 1);
            const std::vector<int64_t> sizes = sa_given ? attr_split : host_ints(s, "Split: the split input");
            OutputList o;
            const auto pieces = op->pieces(x.size(a), sa_given || s ? &sizes : nullptr);
            for (size_t k = 0; k < pieces.size(); k++) {
                const std::vector<SliceRange> r = Split::piece_ranges(x, a, pieces[k]);
                if (x.host() && k < caches.size()) o.push_back(materialize(c, hostops::slice(*x.host(), r), *caches[k]));
                else o.push_back(slice_tensor(c, x, r));
            }
            return o;
        };
    }

    // GRU / LSTM: attributes through read_rnn_node (public: what the reference refuses at load is refused here, device or not); unnamed outputs are not
    // computed.  Rows of the batch are independent (not batch_coupled); the workspace is the context's auxiliary scratch, sized by the warm-up run before a capture.
    void make_rnn_step(Step &st, const onnx::Node &n) {
        const RnnNode a = read_rnn_node(n, st.name);
        if (a.lstm) {
            auto op = std::make_shared<LSTM>();
            op->direction = a.direction; op->hidden_size = a.hidden_size; op->output_mask = a.output_mask;
            run_plainly(st, op);
        } else {
            auto op = std::make_shared<GRU>();
            op->direction = a.direction; op->hidden_size = a.hidden_size; op->output_mask = a.output_mask; op->linear_before_reset = true;
            run_plainly(st, op);
        }
    }

    // Shape-only operators: the output aliases the input's buffer (src/ops/layout.rs reshapes in place when it can).
    void make_view_step(Step &st, const onnx::Node &n) {
        const std::string kind = n.op_type;
        const int axis = (int)n.get_int("axis", 1);
        std::vector<int64_t> spec; // Reshape target / (Un)Squeeze axes from a constant input (opset >= 13) or the attribute
        bool have_spec = false;
        bool runtime_spec = false; // the shape / axes operand is computed by the graph (shape arithmetic): read from its host value at run time
        if (n.inputs.size() > 1 && !n.inputs[1].empty()) {
            if (!is_const(n.inputs[1])) {
                runtime_spec = true;
                st.in.resize(2);
            } else {
                for (int32_t v : const_of(n.inputs[1]).to_host<int32_t>()) spec.push_back(v);
                st.in.resize(1);
            }
            have_spec = true;
        } else if (const onnx::Attr *a = n.attr("axes")) { spec = a->ints; have_spec = true; }
        else if (const onnx::Attr *a2 = n.attr("shape")) { spec = a2->ints; have_spec = true; }
        const bool allowzero = n.get_int("allowzero", 0) != 0;
        st.kind_name = kind + "(view)";
        const std::string step_name = st.name;
        st.run = [kind, axis, spec_const = spec, have_spec, allowzero, runtime_spec, step_name](Context &, const InputList &in) {
            const Tensor &x = require(in, 0);
            const std::vector<int64_t> spec_rt = runtime_spec ? host_ints(&require(in, 1), kind + " " + step_name + ": the shape / axes input") : std::vector<int64_t>();
            const std::vector<int64_t> &spec = runtime_spec ? spec_rt : spec_const;
            const std::vector<int64_t> s = hostops::view_shape(kind, x.shape(), spec, have_spec, axis, allowzero);
            OutputList out;
            out.push_back(Tensor::view_of(x, s));
            if (x.host()) out.back().set_host(std::make_shared<const HostVal>(hostops::reshaped(*x.host(), s))); // the same values under the new shape
            return out;
        };
        st.view = true;
    }

    // Reference counts per value (Graph::run_plan's temp value refcounts): a value's buffer returns to the pool after its
    // last consumer; a view adds one use to its base that is released together with the view itself.
    void plan_liveness() {
        uses_.assign(names_.size(), 0);
        std::vector<int> base_of(names_.size(), -1);
        for (auto &o : outputs_) uses_[(size_t)ids_.at(o.name)] += 1 << 20; // never released
        for (auto &st : steps_) {
            for (int id : st.in) if (id >= 0) uses_[(size_t)id]++;
            if (st.view && st.in[0] >= 0 && st.out[0] >= 0) {
                int base = st.in[0];
                while (base_of[(size_t)base] >= 0) base = base_of[(size_t)base];
                base_of[(size_t)st.out[0]] = base;
                uses_[(size_t)base]++; // held by the view
            }
        }
        std::vector<int> left(uses_);
        for (auto &st : steps_) {
            for (int id : st.in) {
                if (id < 0 || consts_.count(id)) continue;
                st.release_after.push_back(id);
                if (--left[(size_t)id] == 0 && base_of[(size_t)id] >= 0) { // the view died: drop its hold on the base
                    st.release_after.push_back(base_of[(size_t)id]);
                    left[(size_t)base_of[(size_t)id]]--;
                }
            }
            // outputs nobody reads (e.g. unused secondary outputs) die immediately
            for (int id : st.out) if (id >= 0 && uses_[(size_t)id] == 0) { uses_[(size_t)id] = 1; st.release_after.push_back(id); }
        }
    }
};

} // namespace rten_hip
