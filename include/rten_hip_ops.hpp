// rten_hip_ops.hpp -- C++ host side above the C ABI (include/rten_hip.h): the reference's operator interface for the hot
// path, mirrored in C++ because the reference is compiled code and its own toolchain (Rust) is not in this image.
//
// What is mirrored (same names, attribute meaning, input order, validation order and OpError messages, which the
// reference's tests assert verbatim -- src/ops/conv.rs:1182-1268, src/ops/matmul.rs:1284-1333):
//   * `Operator` / `OpRunContext` / `OpRegistry`   src/operator.rs:486-613, src/op_registry.rs:25-72
//   * `OpError`                                    src/operator.rs:116-144
//   * Conv, ConvInteger, ConvIntegerToFloat        src/ops/conv.rs:367-403, 478-587
//   * MatMul, FusedMatMul, Gemm, MatMulInteger(ToFloat)   src/ops/matmul.rs:106-156, 387-510, 582-810
//   * Softmax, LayerNormalization                  src/ops/norm.rs:456-529, 825-840
//   * Gelu, Erf, Relu, Add, Mul                    src/ops/unary_elementwise.rs, binary_elementwise.rs:476-495
//   * MaxPool, AveragePool, GlobalAveragePool      src/ops/pooling.rs:174-521
//   * DynamicQuantizeLinear                        src/ops/quantize.rs:352-436
//   * Einsum, ReduceSum                            src/ops/einsum.rs:21-692, src/ops/reduce.rs:414-520,1126-1165
//   * Resize, Upsample, Split                      src/ops/resize.rs:273-652, src/ops/split.rs:34-136
// Validation runs on the host before any launch; arithmetic is done by librten_hip.so on device-resident tensors.  There
// is no CPU fallback: without a gfx950 device `Context` throws.  Header only; C++17.
#pragma once
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <numeric>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "rten_hip.h"

namespace rten_hip {

// ---- OpError (src/operator.rs:116-144)
struct OpError : std::runtime_error {
    enum Kind { InvalidValue, IncompatibleInputShapes, UnsupportedValue, UnsupportedType, MissingInputs, InputCastFailed, BackendUnavailable, Hip };
    Kind kind;
    std::string msg;
    OpError(Kind k, std::string m) : std::runtime_error(kind_name(k) + (m.empty() ? "" : "(\"" + m + "\")")), kind(k), msg(std::move(m)) {}
    static std::string kind_name(Kind k) {
        static const char *n[] = {"InvalidValue", "IncompatibleInputShapes", "UnsupportedValue", "UnsupportedType", "MissingInputs", "InputCastFailed",
                                  "BackendUnavailable", "Hip"};
        return n[k];
    }
};

// ---- Context: RAII over rten_hip_ctx.  May be shared by host threads (rten_hip.h, "Thread safety"): the C ABI locks the
// context per call and the buffer pool below has its own mutex.
class Context {
  public:
    explicit Context(int device = 0, void *stream = nullptr) {
        const int32_t rc = rten_hip_init(device, stream, &h_);
        if (rc == RTEN_HIP_ERR_NO_DEVICE) throw OpError(OpError::BackendUnavailable, "no usable gfx950 (MI355X) device: the HIP backend has no CPU fallback");
        if (rc != RTEN_HIP_OK) throw OpError(OpError::Hip, "rten_hip_init failed");
    }
    // Borrows a context created elsewhere (a C-ABI caller's): same stream, same lock; never destroyed here.
    struct Borrow {};
    Context(rten_hip_ctx *borrowed, Borrow) : h_(borrowed), owned_(false) {
        if (!borrowed) throw OpError(OpError::InvalidValue, "null context");
    }
    ~Context() { if (h_) { for (auto &b : parked_) rten_hip_free(h_, b.first); trim_pool(); if (one_) rten_hip_free(h_, one_); if (zero_) rten_hip_free(h_, zero_); if (owned_) rten_hip_destroy(h_); } }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    rten_hip_ctx *raw() const { return h_; }
    void sync() { check(rten_hip_sync(h_)); }

    // Device buffer pool (src/buffer_pool.rs: operators take output buffers from the pool, the executor returns dead values
    // to it).  Off by default; a graph executor turns it on so that steady-state runs allocate nothing.  Buffers are handed
    // out by exact byte size; the stream orders reuse (one stream per context).
    void enable_pool(bool on = true) { pool_on_ = on; if (!on) trim_pool(); }
    void *alloc(size_t bytes) {
        if (pool_on_) {
            std::lock_guard<std::mutex> lk(pool_mu_);
            auto it = pool_.find(bytes);
            if (it != pool_.end() && !it->second.empty()) { void *p = it->second.back(); it->second.pop_back(); return p; }
        }
        void *p = nullptr;
        check(rten_hip_malloc(h_, bytes, &p));
        return p;
    }
    // A buffer that does NOT come from the pool (it returns to it when released): for values that outlive the run that makes them -- taken from the pool,
    // such a buffer would leave the next run one buffer of its size short.
    void *alloc_unpooled(size_t bytes) {
        void *p = nullptr;
        check(rten_hip_malloc(h_, bytes, &p));
        return p;
    }
    void release(void *p, size_t bytes) {
        if (!p) return;
        if (pool_on_) { std::lock_guard<std::mutex> lk(pool_mu_); pool_[bytes].push_back(p); }
        else rten_hip_free(h_, p);
    }
    void trim_pool() {
        std::lock_guard<std::mutex> lk(pool_mu_);
        for (auto &kv : pool_) for (void *p : kv.second) rten_hip_free(h_, p);
        pool_.clear();
    }
    // ---- device copies a step keeps ACROSS runs (a host-evaluated step's cached constants, Div's reciprocals) and captured hipGraphs.  A captured graph has
    // the address of every such copy it read baked in, so a copy that existed when a capture was made must neither be freed nor reach the pool while any
    // capture on this context is alive.  A cache stamps each copy when it makes it (`stamp`), an executor reports its captures (`capture_made` /
    // `capture_destroyed`), and a cache that evicts a copy hands the buffer to `retire`: it is parked if a live capture may know it, released otherwise, and
    // everything parked is released when the last capture is destroyed.  Bound: a cache keeps at most 8 copies, so at most 8 copies per caching step are parked
    // per capture made since the context last had none alive; copies made AFTER the latest capture are evicted as before.
    uint64_t stamp() { std::lock_guard<std::mutex> lk(pool_mu_); return ++clock_; }
    void capture_made() { std::lock_guard<std::mutex> lk(pool_mu_); live_captures_++; pinned_before_ = ++clock_; }
    void capture_destroyed() {
        std::vector<std::pair<void *, size_t>> parked;
        {
            std::lock_guard<std::mutex> lk(pool_mu_);
            if (live_captures_ == 0 || --live_captures_ > 0) return;
            pinned_before_ = 0;
            parked.swap(parked_);
        }
        for (auto &b : parked) release(b.first, b.second);
    }
    void retire(void *p, size_t bytes, uint64_t born) {
        if (!p) return;
        {
            std::lock_guard<std::mutex> lk(pool_mu_);
            if (live_captures_ > 0 && born < pinned_before_) { parked_.emplace_back(p, bytes); return; }
        }
        release(p, bytes);
    }
    const int32_t *zero_i32() { // device-resident int32 0 (x + 0: a raw-word move through the generic element-wise kernel)
        if (!zero_) {
            const int32_t v = 0;
            check(rten_hip_malloc(h_, 4, &zero_));
            check(rten_hip_memcpy_h2d(h_, zero_, &v, 4));
        }
        return (const int32_t *)zero_;
    }
    const float *one() { // device-resident 1.0f (x * 1.0f is exact: Cast as cast_scale)
        if (!one_) {
            const float v = 1.0f;
            check(rten_hip_malloc(h_, 4, &one_));
            check(rten_hip_memcpy_h2d(h_, one_, &v, 4));
        }
        return (const float *)one_;
    }
    // maps ABI status codes onto OpError variants (include/rten_hip.h, "status codes")
    void check(int32_t rc) const {
        if (rc == RTEN_HIP_OK) return;
        const std::string m = rten_hip_last_error(h_);
        switch (rc) {
        case RTEN_HIP_ERR_INVALID_VALUE: throw OpError(OpError::InvalidValue, m);
        case RTEN_HIP_ERR_INCOMPATIBLE_SHAPES: throw OpError(OpError::IncompatibleInputShapes, m);
        case RTEN_HIP_ERR_UNSUPPORTED: throw OpError(OpError::UnsupportedValue, m);
        default: throw OpError(OpError::Hip, m);
        }
    }

  private:
    rten_hip_ctx *h_ = nullptr;
    bool owned_ = true;
    bool pool_on_ = false;
    void *one_ = nullptr, *zero_ = nullptr;
    std::map<size_t, std::vector<void *>> pool_;
    std::mutex pool_mu_; // the pool is shared by concurrent Model::run callers (the C ABI context locks itself)
    uint64_t clock_ = 0, pinned_before_ = 0; // stamps of kept copies; copies stamped before `pinned_before_` may be known to a live capture
    size_t live_captures_ = 0;
    std::vector<std::pair<void *, size_t>> parked_;
};

// ---- device tensor (the backend's `Value`: contiguous, row-major, device resident)
enum class DType { F32, I32, U8, I8 };
inline size_t dtype_size(DType t) { return (t == DType::F32 || t == DType::I32) ? 4 : 1; }

// A small tensor whose VALUES the host knows (shape arithmetic: the output of Shape, constants, and what Gather / Concat / Slice / Unsqueeze / arithmetic /
// comparisons make of them).  The reference folds such subgraphs at load (`propagate_constants`, src/optimize.rs:705, over its symbolic shapes); here
// the executor evaluates them on the host at run time (rten_hip_graph.hpp: no device work, nothing of it in a captured hipGraph) and attaches the
// result to the device tensor that carries the value, so that Reshape / Expand / Slice / ConstantOfShape read their shape operands without a
// device round trip.  Integers and booleans are int32-valued (onnx_loader.rs:332-339), kept in int64 for the arithmetic.
struct HostVal {
    std::vector<int64_t> shape;
    bool is_float = false;
    std::vector<int64_t> i;
    std::vector<float> f;
    int64_t len() const { int64_t n = 1; for (int64_t d : shape) n *= d; return n; }
    bool operator==(const HostVal &o) const {
        if (shape != o.shape || is_float != o.is_float || i != o.i || f.size() != o.f.size()) return false;
        return f.empty() || std::memcmp(f.data(), o.f.data(), f.size() * sizeof(float)) == 0; // bitwise (NaN payloads, -0)
    }
};

class Tensor {
  public:
    Tensor() = default;
    Tensor(Context &ctx, std::vector<int64_t> shape, DType dt) : ctx_(&ctx), shape_(std::move(shape)), dtype_(dt) {
        cap_ = bytes() ? bytes() : 4;
        ptr_ = ctx.alloc(cap_);
    }
    // Shape plus an explicit byte capacity (>= bytes()): opaque device layouts that are larger than the logical tensor,
    // e.g. the int8 kernel's zero-point-padded staged image of an [N, C, H, W] activation.
    Tensor(Context &ctx, std::vector<int64_t> shape, DType dt, size_t capacity) : ctx_(&ctx), shape_(std::move(shape)), dtype_(dt) {
        cap_ = std::max<size_t>(std::max(capacity, bytes()), 4);
        ptr_ = ctx.alloc(cap_);
    }
    // Non-owning alias of `base`'s storage with another shape (Reshape / Flatten / Squeeze as views, src/ops/layout.rs):
    // the caller keeps `base` alive for as long as the view is used.
    static Tensor view_of(const Tensor &base, std::vector<int64_t> shape) {
        Tensor t;
        t.ctx_ = base.ctx_; t.ptr_ = base.ptr_; t.shape_ = std::move(shape); t.dtype_ = base.dtype_; t.owns_ = false;
        return t;
    }
    // Non-owning alias of `bytes_off` bytes into `base` (a sub-batch slice of a resident full-batch buffer).
    static Tensor view_at(const Tensor &base, size_t bytes_off, std::vector<int64_t> shape) {
        Tensor t = view_of(base, std::move(shape));
        t.ptr_ = (char *)base.ptr_ + bytes_off;
        return t;
    }
    static Tensor view_at(const Tensor &base, size_t bytes_off, std::vector<int64_t> shape, DType dt) { // ... typed: a slot of a byte arena
        Tensor t = view_at(base, bytes_off, std::move(shape));
        t.dtype_ = dt;
        return t;
    }
    template <typename T>
    static Tensor from_host(Context &ctx, std::vector<int64_t> shape, const T *data) {
        Tensor t(ctx, std::move(shape), dtype_of<T>());
        if (t.bytes()) ctx.check(rten_hip_memcpy_h2d(ctx.raw(), t.ptr_, data, t.bytes()));
        return t;
    }
    // ... into a buffer of its own rather than one of the pool's (Context::alloc_unpooled): a value a step keeps across runs
    template <typename T>
    static Tensor from_host_unpooled(Context &ctx, std::vector<int64_t> shape, const T *data) {
        Tensor t;
        t.ctx_ = &ctx; t.shape_ = std::move(shape); t.dtype_ = dtype_of<T>();
        t.cap_ = std::max<size_t>(t.bytes(), 4);
        t.ptr_ = ctx.alloc_unpooled(t.cap_);
        if (t.bytes()) ctx.check(rten_hip_memcpy_h2d(ctx.raw(), t.ptr_, data, t.bytes()));
        return t;
    }
    ~Tensor() { release(); }
    Tensor(Tensor &&o) noexcept { *this = std::move(o); }
    Tensor &operator=(Tensor &&o) noexcept {
        if (this != &o) { release(); ctx_ = o.ctx_; ptr_ = o.ptr_; shape_ = std::move(o.shape_); dtype_ = o.dtype_; cap_ = o.cap_; owns_ = o.owns_; host_ = std::move(o.host_); uniform_ = o.uniform_; o.ptr_ = nullptr; }
        return *this;
    }
    Tensor(const Tensor &) = delete;
    Tensor &operator=(const Tensor &) = delete;

    const std::vector<int64_t> &shape() const { return shape_; }
    int64_t size(int i) const { return shape_[(size_t)i]; }
    int ndim() const { return (int)shape_.size(); }
    int64_t len() const { return std::accumulate(shape_.begin(), shape_.end(), (int64_t)1, std::multiplies<int64_t>()); }
    size_t bytes() const { return (size_t)len() * dtype_size(dtype_); }
    DType dtype() const { return dtype_; }
    void *ptr() const { return ptr_; }
    bool owns() const { return owns_; } // false for view_of / view_at aliases: somebody else keeps the storage alive
    // Gives up a copy a step kept across runs (stamped `born` when it was made): Context::retire parks the buffer while a captured graph may know its address
    void retire(uint64_t born) { if (ptr_ && ctx_ && owns_) ctx_->retire(ptr_, cap_, born); ptr_ = nullptr; }
    template <typename T> std::vector<T> to_host() const {
        std::vector<T> out((size_t)len());
        if (bytes()) ctx_->check(rten_hip_memcpy_d2h(ctx_->raw(), out.data(), ptr_, bytes())); // synchronises
        return out;
    }
    void reshape(std::vector<int64_t> s) { shape_ = std::move(s); uniform_ = 0; }
    // Bit d set = every slice along dim d holds the same values (the tensor is a broadcast along d that was materialised): what an element-wise step knows
    // about its result when each operand had size 1 there, was itself uniform there, or is a host value that is.  A consumer that broadcasts along d anyway may
    // then read ONE slice -- the exporter-written attention mask [B, 1, S, T] whose S rows are copies of a [B, 1, 1, T] row takes the fused attention kernel's
    // shared-mask form (round 6).  Fresh tensors and views start at 0 (nothing known).
    uint32_t uniform_dims() const { return uniform_; }
    void set_uniform_dims(uint32_t m) { uniform_ = m; }
    // the host's copy of the values, when it has one (see HostVal); views made with view_of() start without one
    const HostVal *host() const { return host_.get(); }
    const std::shared_ptr<const HostVal> &host_ptr() const { return host_; }
    void set_host(std::shared_ptr<const HostVal> h) { host_ = std::move(h); }

    template <typename T> static DType dtype_of() {
        if (std::is_same<T, float>::value) return DType::F32;
        if (std::is_same<T, int32_t>::value) return DType::I32;
        if (std::is_same<T, uint8_t>::value) return DType::U8;
        return DType::I8;
    }

  private:
    void release() { if (ptr_ && ctx_ && owns_) ctx_->release(ptr_, cap_); ptr_ = nullptr; }
    Context *ctx_ = nullptr;
    void *ptr_ = nullptr;
    size_t cap_ = 0;
    bool owns_ = true;
    std::vector<int64_t> shape_;
    DType dtype_ = DType::F32;
    std::shared_ptr<const HostVal> host_;
    uint32_t uniform_ = 0;
};

// ---- Operator interface (src/operator.rs:486-613).  Optional inputs are null pointers (InputList::get).
using InputList = std::vector<const Tensor *>;
using OutputList = std::vector<Tensor>;

inline const Tensor &require(const InputList &in, size_t i) {
    if (i >= in.size() || !in[i]) throw OpError(OpError::MissingInputs, "");
    return *in[i];
}
inline const Tensor *get(const InputList &in, size_t i) { return i < in.size() ? in[i] : nullptr; }
inline const Tensor &want(const Tensor &t, DType dt, const char *what) {
    if (t.dtype() != dt) throw OpError(OpError::InputCastFailed, std::string("expected ") + what + " tensor");
    return t;
}
inline void *vp(const Tensor *t) { return t ? t->ptr() : nullptr; }

class Operator {
  public:
    virtual ~Operator() = default;
    virtual const char *name() const = 0;
    virtual int max_inputs() const { return -1; } // < 0: unbounded (Operator::max_inputs -> None)
    virtual OutputList run(Context &ctx, const InputList &inputs) const = 0;
};

// Padding::Same / Padding::Fixed (src/ops/mod.rs)
struct Padding {
    bool same = false;
    std::vector<int> fixed{0, 0, 0, 0};
    static Padding Same() { Padding p; p.same = true; return p; }
    static Padding Fixed(std::vector<int> v) { Padding p; p.fixed = std::move(v); return p; }
};

struct OutputSize { int oh, ow; int pads[4]; };
// calc_output_size_and_padding (src/ops/pooling.rs:139-159): same error strings through the ABI
inline OutputSize calc_output_size_and_padding(int h, int w, int kh, int kw, const std::vector<int> &strides, const Padding &padding,
                                               const std::vector<int> &dilations = {1, 1}, bool ceil_mode = false) {
    if (!padding.same && padding.fixed.size() != 4) throw OpError(OpError::InvalidValue, "Expected 4 padding values");
    int32_t pads[4] = {0, 0, 0, 0}, out[2], opads[4];
    if (!padding.same) for (int i = 0; i < 4; i++) pads[i] = padding.fixed[(size_t)i];
    const char *msg = nullptr;
    const int32_t rc = rten_hip_calc_output_size_and_padding(h, w, kh, kw, strides[0], strides[1], padding.same ? 1 : 0, pads, dilations[0], dilations[1],
                                                             ceil_mode ? 1 : 0, out, opads, &msg);
    if (rc) throw OpError(OpError::InvalidValue, msg ? msg : "");
    return OutputSize{out[0], out[1], {opads[0], opads[1], opads[2], opads[3]}};
}

// Launch plan of the f32 GEMM / implicit-GEMM conv kernels: tile variant, exact split-K mode and group count, tile
// order (rten_hip_set_gemm_variant_override / _split / _order).  Unset = the backend's automatic choice.  An executor
// picks one per layer by measurement at load time, as the reference picks its kernel per ISA (rten-gemm/src/lib.rs:534-547).
struct GemmPlan {
    bool set = false;
    int variant = -1, mode = 3, groups = 1, order = 0;
};
class PlanScope { // applies a plan around one call and restores the automatic plan afterwards
  public:
    PlanScope(Context &ctx, const GemmPlan &p) : ctx_(ctx), on_(p.set) {
        if (!on_) return;
        ctx.check(rten_hip_tuning_save(ctx.raw(), saved_)); // (the context may be a caller's: its knobs come back as they were, not as defaults)
        ctx.check(rten_hip_set_gemm_variant_override(ctx.raw(), p.variant));
        ctx.check(rten_hip_set_gemm_split(ctx.raw(), p.mode, p.groups));
        ctx.check(rten_hip_set_gemm_order(ctx.raw(), p.order));
    }
    ~PlanScope() {
        if (!on_) return;
        rten_hip_tuning_restore(ctx_.raw(), saved_);
    }

  private:
    Context &ctx_;
    bool on_;
    int32_t saved_[8] = {};
};

// ------------------------------------------------------------------------------------------------ activations with parameters
// An element-wise activation (RTEN_HIP_ACT_* kind and its parameters): the standalone operators below, and the epilogue that
// Conv / FusedMatMul apply after their bias (and residual).
struct Activation {
    int32_t kind = RTEN_HIP_ACT_NONE;
    float alpha = 0.f, beta = 0.f;
};
inline const char *activation_name(int32_t kind) {
    static const char *n[] = {"", "Relu", "Gelu", "Sigmoid", "Silu", "Swish", "HardSigmoid", "HardSwish", "Clip", "LeakyRelu", "Elu"};
    return kind >= 0 && kind <= RTEN_HIP_ACT_ELU ? n[kind] : "?";
}

// ------------------------------------------------------------------------------------------------ Conv
struct Conv : Operator {
    GemmPlan plan;
    int groups = 1;
    std::vector<int> dilations{1, 1};
    Padding padding;
    std::vector<int> strides{1, 1};
    bool fuse_relu = false; // backend fusion of the following Relu; a 4th input is the residual Add operand
    Activation act;         // backend fusion of another following activation (Sigmoid, Silu, Clip, ...); exclusive with fuse_relu

    const char *name() const override { return "Conv"; }
    int max_inputs() const override { return 4; }

    // shape checks in the reference's order with its messages (src/ops/conv.rs:136-214)
    rten_hip_conv2d_desc geometry(const std::vector<int64_t> &xs, const std::vector<int64_t> &ws) const {
        if (xs.size() != 4) throw OpError(OpError::InvalidValue, "input must have 4 dims (NCHW)");
        if (ws.size() != 4) throw OpError(OpError::InvalidValue, "kernel must have 4 dims (OCHW)");
        if (strides.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 stride values");
        if (dilations.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 dilation values");
        const int n = (int)xs[0], c = (int)xs[1], h = (int)xs[2], w = (int)xs[3];
        const int o = (int)ws[0], kc = (int)ws[1], kh = (int)ws[2], kw = (int)ws[3];
        const OutputSize os = calc_output_size_and_padding(h, w, kh, kw, strides, padding, dilations);
        if (groups == 0) throw OpError(OpError::InvalidValue, "Group count must be > 0");
        if (c % groups != 0) throw OpError(OpError::InvalidValue, "Input channel count not divisible by groups");
        if (c / groups != kc) throw OpError(OpError::IncompatibleInputShapes, "Input channels (per group) does not match kernel input channels");
        if (o % groups != 0) throw OpError(OpError::InvalidValue, "Output channel count not divisible by groups");
        rten_hip_conv2d_desc d{};
        d.n = n; d.c = c; d.h = h; d.w = w; d.o = o; d.kh = kh; d.kw = kw;
        for (int i = 0; i < 4; i++) d.pads[i] = os.pads[i];
        d.stride_h = strides[0]; d.stride_w = strides[1]; d.dil_h = dilations[0]; d.dil_w = dilations[1];
        d.groups = groups; d.out_h = os.oh; d.out_w = os.ow;
        return d;
    }

    // PrepackedInput analogue (src/operator.rs:25-66): stage the constant weight once
    Tensor prepack(Context &ctx, const Tensor &weight) const {
        rten_hip_conv2d_desc d{};
        d.n = 1; d.c = (int)weight.size(1) * groups; d.h = d.w = 1; d.o = (int)weight.size(0); d.kh = (int)weight.size(2); d.kw = (int)weight.size(3);
        d.stride_h = d.stride_w = d.dil_h = d.dil_w = 1; d.groups = groups; d.out_h = d.out_w = 1;
        Tensor packed(ctx, {(int64_t)(rten_hip_conv2d_f32_packed_bytes(&d) / 4)}, DType::F32);
        ctx.check(rten_hip_conv2d_f32_prepack(ctx.raw(), &d, (const float *)weight.ptr(), (float *)packed.ptr()));
        return packed;
    }

    OutputList run(Context &ctx, const InputList &in) const override { return run_packed(ctx, in, nullptr); }
    OutputList run_packed(Context &ctx, const InputList &in, const Tensor *packed_weight) const {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const Tensor &w = want(require(in, 1), DType::F32, "float32");
        const Tensor *bias = get(in, 2), *residual = get(in, 3);
        if (x.ndim() == 3) { // 1-D convolution: expand to 2-D, remove the extra axis from the result (conv.rs:142-182; views only)
            if (w.ndim() != 3) throw OpError(OpError::InvalidValue, "kernel must have 3 dims (OCW)");
            Conv op2 = *this;
            if (!padding.same) {
                if (padding.fixed.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 pad values");
                op2.padding = Padding::Fixed({0, padding.fixed[0], 0, padding.fixed[1]});
            }
            if (strides.size() != 1) throw OpError(OpError::InvalidValue, "expected 1 stride value");
            if (dilations.size() != 1) throw OpError(OpError::InvalidValue, "expected 1 dilation value");
            op2.strides = {1, strides[0]};
            op2.dilations = {1, dilations[0]};
            const Tensor x2 = Tensor::view_of(x, {x.size(0), x.size(1), 1, x.size(2)}), w2 = Tensor::view_of(w, {w.size(0), w.size(1), 1, w.size(2)});
            Tensor r2;
            if (residual) r2 = Tensor::view_of(*residual, {residual->size(0), residual->size(1), 1, residual->size(2)});
            OutputList out = op2.run_packed(ctx, {&x2, &w2, bias, residual ? &r2 : nullptr}, packed_weight);
            out[0].reshape({out[0].size(0), out[0].size(1), out[0].size(3)});
            return out;
        }
        const rten_hip_conv2d_desc d = geometry(x.shape(), w.shape());
        if (bias && bias->size(0) != d.o) throw OpError(OpError::IncompatibleInputShapes, "bias.size(0) != out_channels");
        Tensor y(ctx, {d.n, d.o, d.out_h, d.out_w}, DType::F32);
        if (fuse_relu && act.kind != RTEN_HIP_ACT_NONE) throw OpError(OpError::InvalidValue, "Conv: fuse_relu and act are exclusive");
        const uint32_t flags = (fuse_relu ? RTEN_HIP_CONV_RELU : 0u) | (residual ? RTEN_HIP_CONV_RESIDUAL : 0u);
        PlanScope scope(ctx, plan);
        const float *wp = (const float *)(packed_weight ? packed_weight->ptr() : w.ptr());
        if (act.kind != RTEN_HIP_ACT_NONE)
            ctx.check(rten_hip_conv2d_f32_act(ctx.raw(), &d, (const float *)x.ptr(), wp, packed_weight ? 1 : 0, (const float *)vp(bias), (const float *)vp(residual), flags,
                                              act.kind, act.alpha, act.beta, (float *)y.ptr()));
        else
            ctx.check(rten_hip_conv2d_f32(ctx.raw(), &d, (const float *)x.ptr(), wp, packed_weight ? 1 : 0, (const float *)vp(bias), (const float *)vp(residual), flags,
                                          (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ ConvTranspose
struct ConvTranspose : Operator { // src/ops/conv_transpose.rs:414-458; kernel layout [C, O/g, kh, kw]
    Padding padding;
    int groups = 1;
    std::vector<int> strides{1, 1}, dilations{1, 1}, output_padding; // output_padding empty = zeros
    const char *name() const override { return "ConvTranspose"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32"), &w = want(require(in, 1), DType::F32, "float32");
        const Tensor *bias = get(in, 2);
        if (x.ndim() == 3) { // 1-D: expand to 2-D, remove the extra axis from the result (conv_transpose.rs:237-291)
            if (w.ndim() != 3) throw OpError(OpError::InvalidValue, "kernel must have 3 dims (OCW)");
            ConvTranspose op2 = *this;
            if (!padding.same) {
                if (padding.fixed.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 pad values");
                op2.padding = Padding::Fixed({0, padding.fixed[0], 0, padding.fixed[1]});
            }
            if (strides.size() != 1) throw OpError(OpError::InvalidValue, "expected 1 stride value");
            if (dilations.size() != 1) throw OpError(OpError::InvalidValue, "expected 1 dilation value");
            if (!output_padding.empty() && output_padding.size() != 1) throw OpError(OpError::InvalidValue, "expected 1 output_padding value");
            op2.strides = {1, strides[0]};
            op2.dilations = {1, dilations[0]};
            if (!output_padding.empty()) op2.output_padding = {0, output_padding[0]};
            const Tensor x2 = Tensor::view_of(x, {x.size(0), x.size(1), 1, x.size(2)}), w2 = Tensor::view_of(w, {w.size(0), w.size(1), 1, w.size(2)});
            OutputList out = op2.run(ctx, {&x2, &w2, bias});
            out[0].reshape({out[0].size(0), out[0].size(1), out[0].size(3)});
            return out;
        }
        if (groups == 0) throw OpError(OpError::InvalidValue, "Group count must be > 0");
        if (x.ndim() != 4) throw OpError(OpError::InvalidValue, "input must have 4 dims (NCHW)");
        if (w.ndim() != 4) throw OpError(OpError::InvalidValue, "kernel must have 4 dims (COHW)");
        const int64_t o = w.size(1) * groups;
        if (bias && bias->size(0) != o) throw OpError(OpError::IncompatibleInputShapes, "bias.size(0) != out_channels");
        if (x.size(1) != w.size(0)) throw OpError(OpError::IncompatibleInputShapes, "Input channels does not match kernel input channels");
        if (w.size(0) % groups != 0) throw OpError(OpError::InvalidValue, "Input channel count not divisible by groups");
        if (strides.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 stride values");
        if (dilations.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 dilation values");
        if (!output_padding.empty() && output_padding.size() != 2) throw OpError(OpError::InvalidValue, "expected 2 output_padding values");
        if (!padding.same && padding.fixed.size() != 4) throw OpError(OpError::InvalidValue, "Wrong number of pad values");
        int32_t pads[4] = {0, 0, 0, 0}, out_hw[2], out_pads[4];
        if (!padding.same) for (int i = 0; i < 4; i++) pads[i] = padding.fixed[(size_t)i];
        const char *msg = nullptr;
        if (rten_hip_conv_transpose_output_size((int)x.size(2), (int)x.size(3), (int)w.size(2), (int)w.size(3), strides[0], strides[1], padding.same ? 1 : 0, pads, dilations[0],
                                                dilations[1], output_padding.empty() ? 0 : output_padding[0], output_padding.empty() ? 0 : output_padding[1], out_hw, out_pads, &msg))
            throw OpError(OpError::InvalidValue, msg ? msg : "");
        rten_hip_conv2d_desc d{};
        d.n = (int)x.size(0); d.c = (int)x.size(1); d.h = (int)x.size(2); d.w = (int)x.size(3); d.o = (int)o; d.kh = (int)w.size(2); d.kw = (int)w.size(3);
        for (int i = 0; i < 4; i++) d.pads[i] = out_pads[i];
        d.stride_h = strides[0]; d.stride_w = strides[1]; d.dil_h = dilations[0]; d.dil_w = dilations[1]; d.groups = groups; d.out_h = out_hw[0]; d.out_w = out_hw[1];
        Tensor y(ctx, {d.n, d.o, d.out_h, d.out_w}, DType::F32);
        ctx.check(rten_hip_conv_transpose2d_f32(ctx.raw(), &d, (const float *)x.ptr(), (const float *)w.ptr(), (const float *)vp(bias), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// zero_point_to_vec (src/ops/matmul.rs:513-531)
inline int zero_point_len(const Tensor *zp, int64_t expected) {
    // zero_point_to_vec, src/ops/matmul.rs:513-531
    if (!zp) return 0;
    if (zp->ndim() == 0) return 1;
    if (zp->ndim() == 1) {
        if (zp->len() != expected) throw OpError(OpError::InvalidValue, "Zero point has incorrect size");
        return (int)expected;
    }
    throw OpError(OpError::UnsupportedValue, "Only scalar or vector zero points are supported");
}

struct ConvInteger : Operator {
    Conv conv; // geometry attributes (groups, dilations, padding, strides)
    int pad_mode = RTEN_HIP_PAD_RAW0_I8; // value of padded taps; x86 reference default
    const char *name() const override { return "ConvInteger"; }
    int max_inputs() const override { return 4; }

    rten_hip_conv2d_int8_desc desc(const Tensor &x, const Tensor &w, const Tensor *x_zp, const Tensor *w_zp) const {
        auto is8 = [](DType t) { return t == DType::U8 || t == DType::I8; };
        if (!is8(x.dtype()) || !is8(w.dtype())) throw OpError(OpError::UnsupportedType, "");
        if (x_zp && x_zp->len() != 1) throw OpError(OpError::InvalidValue, "input zero point must be a scalar");
        const int wz = zero_point_len(w_zp, w.ndim() ? w.size(0) : 0);
        rten_hip_conv2d_int8_desc di{};
        di.conv = conv.geometry(x.shape(), w.shape());
        di.x_signed = x.dtype() == DType::I8; di.w_signed = w.dtype() == DType::I8; di.w_zp_len = wz; di.pad_mode = pad_mode;
        return di;
    }
    OutputList run(Context &ctx, const InputList &in) const override { return run_fused(ctx, in, nullptr, nullptr, nullptr, false); }

    // PrepackedInput analogue for constant weights (rten_hip_conv2d_int8_prepack); an empty tensor (len 0) when the staged
    // kernel does not cover the geometry -- pass the plain weights then.
    Tensor prepack(Context &ctx, const Tensor &w) const {
        rten_hip_conv2d_int8_desc di{};
        di.conv.n = 1; di.conv.c = (int)w.size(1) * conv.groups; di.conv.o = (int)w.size(0); di.conv.kh = (int)w.size(2); di.conv.kw = (int)w.size(3);
        di.conv.h = di.conv.kh; di.conv.w = di.conv.kw; di.conv.out_h = di.conv.out_w = 1;
        di.conv.stride_h = di.conv.stride_w = di.conv.dil_h = di.conv.dil_w = 1; di.conv.groups = conv.groups;
        di.w_signed = w.dtype() == DType::I8;
        const size_t nbytes = rten_hip_conv2d_int8_packed_bytes(&di);
        if (!nbytes) return Tensor(ctx, {0}, DType::U8);
        Tensor packed(ctx, {(int64_t)nbytes}, DType::U8);
        ctx.check(rten_hip_conv2d_int8_prepack(ctx.raw(), &di, w.ptr(), packed.ptr()));
        return packed;
    }

    // Options of the staged pipeline: prepacked weights, `x` already in the kernel's staged layout
    // (written by DynamicQuantizeLinearStaged below; its logical shape is still [N, C, H, W]), and a statistics block in
    // which the epilogue accumulates min/max of the f32 outputs for the DynamicQuantizeLinear that consumes them.
    struct Staging {
        const Tensor *packed_weight = nullptr;
        bool x_staged = false;
        void *stats_out = nullptr;
    };

    // scale != null: ConvIntegerToFloat epilogue (cast_scale, then the following Add(bias) / Add(residual) / Relu)
    OutputList run_fused(Context &ctx, const InputList &in, const Tensor *scale, const Tensor *bias, const Tensor *residual, bool relu) const {
        return run_staged(ctx, in, scale, bias, residual, relu, Staging());
    }
    // per_channel_scale: `scale` holds one value per output channel ([1,O,1,1] / [O,1,1], the Cast -> Mul form of per-channel weights)
    OutputList run_staged(Context &ctx, const InputList &in, const Tensor *scale, const Tensor *bias, const Tensor *residual, bool relu,
                          const Staging &sg, bool per_channel_scale = false) const {
        const Tensor &x = require(in, 0), &w = require(in, 1);
        const Tensor *x_zp = get(in, 2), *w_zp = get(in, 3);
        rten_hip_conv2d_int8_desc di = desc(x, w, x_zp, w_zp);
        const bool packed = sg.packed_weight && sg.packed_weight->len() > 0;
        di.weights_packed = packed ? 1 : 0;
        di.x_staged = sg.x_staged ? 1 : 0;
        if (scale && per_channel_scale) {
            if (scale->len() != di.conv.o) throw OpError(OpError::IncompatibleInputShapes, "per-channel scale length does not match output channels");
            di.scale_len = di.conv.o;
        }
        if (bias && bias->len() != di.conv.o) throw OpError(OpError::IncompatibleInputShapes, "bias length does not match output channels");
        Tensor y(ctx, {di.conv.n, di.conv.o, di.conv.out_h, di.conv.out_w}, scale ? DType::F32 : DType::I32);
        const uint32_t flags = (relu ? RTEN_HIP_CONV_RELU : 0u) | (residual ? RTEN_HIP_CONV_RESIDUAL : 0u);
        const void *wp = packed ? sg.packed_weight->ptr() : w.ptr();
        if (sg.stats_out && scale)
            ctx.check(rten_hip_conv2d_int8_stats(ctx.raw(), &di, x.ptr(), wp, vp(x_zp), vp(w_zp), (const float *)vp(scale), (const float *)vp(bias),
                                                 (const float *)vp(residual), flags, y.ptr(), sg.stats_out));
        else
        ctx.check(rten_hip_conv2d_int8(ctx.raw(), &di, x.ptr(), wp, vp(x_zp), vp(w_zp), (const float *)vp(scale), (const float *)vp(bias),
                                       (const float *)vp(residual), flags, y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

struct ConvIntegerToFloat : Operator { // src/ops/conv.rs:552-587: inputs X, W, x_zp, w_zp, scale (+ bias, residual: backend fusion)
    ConvInteger conv;
    bool fuse_relu = false;
    const char *name() const override { return "ConvIntegerToFloat"; }
    int max_inputs() const override { return 7; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &scale = want(require(in, 4), DType::F32, "float32");
        if (scale.len() != 1) throw OpError(OpError::InvalidValue, "scale should be a scalar");
        return conv.run_fused(ctx, InputList(in.begin(), in.begin() + 4), &scale, get(in, 5), get(in, 6), fuse_relu);
    }
};

// ------------------------------------------------------------------------------------------------ MatMul family
namespace detail {
inline int64_t prod(const std::vector<int64_t> &v, size_t b, size_t e) {
    int64_t p = 1;
    for (size_t i = b; i < e; i++) p *= v[i];
    return p;
}
// numpy.matmul shape rules (src/ops/matmul.rs:208-385); contiguous inputs; b_transposed folds transB into strides
// act: RTEN_HIP_ACT_NONE / RELU / GELU in the descriptor; any other kind (with act_alpha / act_beta) through rten_hip_gemm_f32_act
inline Tensor matmul(Context &ctx, const Tensor &a, const Tensor &b, const Tensor *bias, float alpha, int act, bool b_transposed, float act_alpha = 0.f,
                     float act_beta = 0.f) {
    std::vector<int64_t> as = a.shape(), bs = b.shape();
    if (as.empty() || bs.empty()) throw OpError(OpError::InvalidValue, "Inputs must have >= 1 dimensions");
    const bool a_vec = as.size() == 1, b_vec = bs.size() == 1;
    if (a_vec) as.insert(as.begin(), 1);
    if (b_vec) { if (b_transposed) bs.insert(bs.begin(), 1); else bs.push_back(1); }
    if (b_transposed) std::swap(bs[bs.size() - 1], bs[bs.size() - 2]);
    const int64_t m = as[as.size() - 2], k = as.back(), kb = bs[bs.size() - 2], n = bs.back();
    if (k != kb) throw OpError(OpError::IncompatibleInputShapes, "Columns of first matrix does not match rows of second matrix");
    const int64_t na = prod(as, 0, as.size() - 2), nb = prod(bs, 0, bs.size() - 2);
    // broadcast the batch prefixes
    std::vector<int64_t> pa(as.begin(), as.end() - 2), pb(bs.begin(), bs.end() - 2), pre;
    const size_t r = std::max(pa.size(), pb.size());
    pa.insert(pa.begin(), r - pa.size(), 1);
    pb.insert(pb.begin(), r - pb.size(), 1);
    for (size_t i = 0; i < r; i++) {
        if (pa[i] != pb[i] && pa[i] != 1 && pb[i] != 1) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast shapes");
        pre.push_back(std::max(pa[i], pb[i]));
    }
    std::vector<int64_t> oshape = pre;
    oshape.push_back(m);
    oshape.push_back(n);
    Tensor y(ctx, oshape, DType::F32);
    if (y.len() > 0) {
        rten_hip_gemm_desc d{};
        d.k = (int)k; d.n = (int)n; d.a_rs = k; d.a_cs = 1; d.b_rs = b_transposed ? 1 : n; d.b_cs = b_transposed ? k : 1; d.ldc = n;
        const bool ext = act > RTEN_HIP_ACT_GELU;
        d.alpha = alpha; d.beta = 0.f; d.bias_kind = bias ? RTEN_HIP_BIAS_PER_COL : RTEN_HIP_BIAS_NONE; d.act = ext ? RTEN_HIP_ACT_NONE : act;
        if (na > 1 && nb == 1) { // matmul.rs:266-297: one [A*M, K] x [K, N] product
            d.m = (int)(na * m); d.batch = 1;
        } else {
            const int64_t batch = prod(pre, 0, pre.size());
            if ((na != 1 && na != batch) || (nb != 1 && nb != batch)) throw OpError(OpError::UnsupportedValue, "partial batch broadcasting is not supported by the device path");
            d.m = (int)m; d.batch = (int)batch; d.a_bs = na > 1 ? m * k : 0; d.b_bs = nb > 1 ? k * n : 0; d.c_bs = m * n;
        }
        if (ext)
            ctx.check(rten_hip_gemm_f32_act(ctx.raw(), &d, (const float *)a.ptr(), (const float *)b.ptr(), (const float *)vp(bias), act, act_alpha, act_beta,
                                            (float *)y.ptr()));
        else
            ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, (const float *)a.ptr(), (const float *)b.ptr(), (const float *)vp(bias), (float *)y.ptr()));
    }
    if (a_vec) oshape.erase(oshape.end() - 2);
    if (b_vec) oshape.pop_back();
    y.reshape(oshape);
    return y;
}
} // namespace detail

struct MatMul : Operator { // src/ops/matmul.rs:387-428
    const char *name() const override { return "MatMul"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        OutputList out;
        out.push_back(detail::matmul(ctx, want(require(in, 0), DType::F32, "float32"), want(require(in, 1), DType::F32, "float32"), nullptr, 1.f, RTEN_HIP_ACT_NONE, false));
        return out;
    }
};

struct FusedMatMul : Operator { // src/ops/matmul.rs:455-510: MatMul + per-column bias + alpha (act: backend fusion of the following activation)
    float alpha = 1.f;
    int act = RTEN_HIP_ACT_NONE; // any RTEN_HIP_ACT_* kind
    float act_alpha = 0.f, act_beta = 0.f;
    bool transpose_b = false;
    const char *name() const override { return "FusedMatMul"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor *bias = get(in, 2);
        if (bias && bias->ndim() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 1 dims");
        OutputList out;
        out.push_back(detail::matmul(ctx, want(require(in, 0), DType::F32, "float32"), want(require(in, 1), DType::F32, "float32"), bias, alpha, act, transpose_b, act_alpha, act_beta));
        return out;
    }
};

struct Gemm : Operator { // src/ops/matmul.rs:106-156: c = alpha * (a b) + beta * c with transA / transB
    float alpha = 1.f, beta = 1.f;
    bool transpose_a = false, transpose_b = false;
    const char *name() const override { return "Gemm"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &a = want(require(in, 0), DType::F32, "float32"), &b = want(require(in, 1), DType::F32, "float32");
        const Tensor *c = get(in, 2);
        if (a.ndim() != 2 || b.ndim() != 2) throw OpError(OpError::InputCastFailed, "expected tensor with 2 dims");
        const int64_t m = transpose_a ? a.size(1) : a.size(0), k = transpose_a ? a.size(0) : a.size(1);
        const int64_t kb = transpose_b ? b.size(1) : b.size(0), n = transpose_b ? b.size(0) : b.size(1);
        if (k != kb) throw OpError(OpError::IncompatibleInputShapes, "Columns of first matrix does not match rows of second matrix");
        // `c` must broadcast to [m, n] (matmul.rs:63-70); the backend takes a row vector [n] or a full matrix
        int bias_kind = RTEN_HIP_BIAS_NONE;
        bool full_c = false;
        if (c) {
            if (c->len() == n && (c->ndim() == 1 || (c->ndim() == 2 && c->size(0) == 1))) bias_kind = RTEN_HIP_BIAS_PER_COL;
            else if (c->ndim() == 2 && c->size(0) == m && c->size(1) == n) full_c = true;
            else throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast c to output shape");
        }
        Tensor y(ctx, {m, n}, DType::F32);
        rten_hip_gemm_desc d{};
        d.m = (int)m; d.n = (int)n; d.k = (int)k; d.batch = 1; d.ldc = n; d.alpha = alpha;
        d.a_rs = transpose_a ? 1 : k; d.a_cs = transpose_a ? m : 1; d.b_rs = transpose_b ? 1 : n; d.b_cs = transpose_b ? k : 1;
        if (full_c) { // output = c; gemm(beta) (matmul.rs:72-82)
            ctx.check(rten_hip_memcpy_d2d(ctx.raw(), y.ptr(), c->ptr(), y.bytes()));
            d.beta = beta;
            ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, (const float *)a.ptr(), (const float *)b.ptr(), nullptr, (float *)y.ptr()));
        } else if (c && beta == 1.f && alpha == 1.f && m != 1) {
            // row vector, c + ab, several rows: the per-column bias epilogue adds in the same place (after the first depth block).  A ONE-row
            // product takes the reference's gemv kernels (rten-gemm/src/lib.rs:668-747,876-891), where the expanded C enters with the
            // FIRST depth block -- ((c + acc0) + acc1) ... -- not after the last: that case runs the general form below.
            d.beta = 0.f; d.bias_kind = bias_kind;
            ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, (const float *)a.ptr(), (const float *)b.ptr(), (const float *)c->ptr(), (float *)y.ptr()));
        } else if (c) { // general case: output = expand(c), then gemm(alpha, beta) (matmul.rs:63-82)
            ctx.check(rten_hip_memset(ctx.raw(), y.ptr(), 0, y.bytes()));
            ctx.check(rten_hip_add_f32(ctx.raw(), y.len(), (const float *)y.ptr(), (const float *)c->ptr(), n, (float *)y.ptr()));
            d.beta = beta;
            ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, (const float *)a.ptr(), (const float *)b.ptr(), nullptr, (float *)y.ptr()));
        } else {
            d.beta = 0.f;
            ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, (const float *)a.ptr(), (const float *)b.ptr(), nullptr, (float *)y.ptr()));
        }
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

struct MatMulInteger : Operator { // src/ops/matmul.rs:582-700 (matmul_integer -> matmul_impl :208-385); scale != null: MatMulIntegerToFloat (:789-794)
    const char *name() const override { return "MatMulInteger"; }
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override { return run_scaled(ctx, in, nullptr); }

    // Operator::prepack for input 1 (matmul.rs:696-705 -> matmul_prepack_b; Graph::prepack_weights, src/graph.rs:488-562): a
    // constant 2-D RHS staged once as the int8 kernel's chunk-major image + column sums.  Returns an empty tensor when the
    // staged kernel does not cover the shape (the op then runs unpacked).
    Tensor prepack(Context &ctx, const Tensor &b) const {
        if ((b.dtype() != DType::U8 && b.dtype() != DType::I8) || b.ndim() != 2) return Tensor();
        const size_t bytes = rten_hip_gemm_int8_packed_bytes((int32_t)b.size(0), (int32_t)b.size(1));
        if (!bytes) return Tensor();
        Tensor packed(ctx, {(int64_t)bytes}, DType::U8);
        ctx.check(rten_hip_gemm_int8_prepack(ctx.raw(), (int32_t)b.size(0), (int32_t)b.size(1), b.ptr(), b.size(1), 1, b.dtype() == DType::I8, packed.ptr()));
        return packed;
    }

    // All of matmul_impl's forms: vector operands (numpy.matmul rules), `[A.., M, K] x [K, N]` collapsed to one product with
    // the row zero points cycled (:259-296), batched / broadcast prefixes (batched_gemm_uninit, :302-372).
    OutputList run_scaled(Context &ctx, const InputList &in, const Tensor *scale, const Tensor *packed_b = nullptr) const {
        const Tensor &a = require(in, 0), &b = require(in, 1);
        auto is8 = [](DType t) { return t == DType::U8 || t == DType::I8; };
        if (!is8(a.dtype()) || !is8(b.dtype())) throw OpError(OpError::UnsupportedType, "");
        const Tensor *a_zp = get(in, 2), *b_zp = get(in, 3);
        const int64_t a_rows = a.ndim() > 1 ? a.size(a.ndim() - 2) : 1, b_cols = b.ndim() > 1 ? b.size(b.ndim() - 1) : 1;
        const int azl = zero_point_len(a_zp, a_rows), bzl = zero_point_len(b_zp, b_cols);
        if (a.ndim() < 1 || b.ndim() < 1) throw OpError(OpError::InvalidValue, "Inputs must have >= 1 dimensions");
        std::vector<int64_t> ash = a.shape(), bsh = b.shape();
        const bool a_vec = ash.size() == 1, b_vec = bsh.size() == 1;
        if (a_vec) ash.insert(ash.begin(), 1);
        if (b_vec) bsh.push_back(1);
        const int64_t m = ash[ash.size() - 2], k = ash.back(), kb = bsh[bsh.size() - 2], n = bsh.back();
        if (k != kb) throw OpError(OpError::IncompatibleInputShapes, "Columns of first matrix does not match rows of second matrix");
        std::vector<int64_t> ap(ash.begin(), ash.end() - 2), bp(bsh.begin(), bsh.end() - 2);
        const size_t np = std::max(ap.size(), bp.size());
        ap.insert(ap.begin(), np - ap.size(), 1);
        bp.insert(bp.begin(), np - bp.size(), 1);
        std::vector<int64_t> op(np);
        for (size_t i = 0; i < np; i++) {
            if (ap[i] != bp[i] && ap[i] != 1 && bp[i] != 1) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast shapes");
            op[i] = (ap[i] == 0 || bp[i] == 0) ? 0 : std::max(ap[i], bp[i]);
        }
        int sl = 0;
        if (scale) {
            if (scale->len() != 1 && scale->len() != n) throw OpError(OpError::IncompatibleInputShapes, "Scale length does not match tensor columns");
            sl = (int)scale->len();
        }
        std::vector<int64_t> out_shape = op;
        if (!a_vec) out_shape.push_back(m);
        if (!b_vec) out_shape.push_back(n);
        Tensor y(ctx, out_shape, scale ? DType::F32 : DType::I32);
        OutputList out;
        if (y.len() == 0) { out.push_back(std::move(y)); return out; }
        auto prod = [](const std::vector<int64_t> &v) { int64_t p = 1; for (int64_t x : v) p *= x; return p; };
        const int64_t num_a = prod(ap), num_b = prod(bp), nb = prod(op);
        const bool packed = packed_b && packed_b->len() && num_b == 1;
        auto call = [&](int64_t mm, int batch, int64_t a_bs, int64_t b_bs, int64_t c_bs, int64_t a_off, int64_t b_off, int64_t c_off) {
            rten_hip_gemm_int8_desc d{};
            d.m = (int)mm; d.n = (int)n; d.k = (int)k; d.a_rs = k; d.a_cs = 1; d.b_rs = n; d.b_cs = 1; d.ldc = n;
            d.a_signed = a.dtype() == DType::I8; d.b_signed = b.dtype() == DType::I8;
            d.a_zp_len = azl; d.b_zp_len = bzl; d.scale_len = sl;
            d.batch = batch; d.a_bs = a_bs; d.b_bs = b_bs; d.c_bs = c_bs; d.b_prepacked = packed ? 1 : 0;
            ctx.check(rten_hip_gemm_int8(ctx.raw(), &d, (const uint8_t *)a.ptr() + a_off, packed ? packed_b->ptr() : (const void *)((const uint8_t *)b.ptr() + b_off), vp(a_zp), vp(b_zp),
                                         (const float *)vp(scale), (uint8_t *)y.ptr() + c_off * 4));
        };
        if (num_b == 1) { // one [A*M, K] x [K, N] product; row r uses a_zp[r % M]
            call(num_a * m, 1, 0, 0, 0, 0, 0, 0);
        } else if ((num_a == 1 || ap == op) && bp == op) {
            call(m, (int)nb, num_a == 1 ? 0 : m * k, k * n, m * n, 0, 0, 0);
        } else { // general broadcast: one product per output matrix
            std::vector<int64_t> as(np), bs(np), idx(np, 0);
            for (size_t i = 0; i < np; i++) {
                int64_t sa = 1, sb = 1;
                for (size_t j = i + 1; j < np; j++) { sa *= ap[j]; sb *= bp[j]; }
                as[i] = ap[i] == 1 ? 0 : sa; bs[i] = bp[i] == 1 ? 0 : sb;
            }
            for (int64_t z = 0; z < nb; z++) {
                int64_t ia = 0, ib = 0;
                for (size_t i = 0; i < np; i++) { ia += idx[i] * as[i]; ib += idx[i] * bs[i]; }
                call(m, 1, 0, 0, 0, ia * m * k, ib * k * n, z * m * n);
                for (size_t i = np; i-- > 0;) { if (++idx[i] < op[i]) break; idx[i] = 0; }
            }
        }
        out.push_back(std::move(y));
        return out;
    }
};

struct MatMulNBits : Operator { // src/ops/matmul/contrib.rs:119-196; the reference op has no K / N fields (they come from the shapes)
    int bits = 4;
    int64_t block_size = 32;
    int accuracy_level = 0; // AccuracyLevel::Int8 (4) is an opt-in approximation the reference may decline (contrib.rs:102-108): always Float here
    const char *name() const override { return "MatMulNBits"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &lhs = want(require(in, 0), DType::F32, "float32");
        const Tensor &rhs = require(in, 1);
        if (rhs.dtype() != DType::U8) throw OpError(OpError::InputCastFailed, "input 1: expected uint8");
        if (rhs.ndim() != 3) throw OpError(OpError::InputCastFailed, "input 1: expected 3 dims");
        const Tensor &scales = want(require(in, 2), DType::F32, "float32");
        const int64_t n = rhs.size(0);
        int64_t k_blocks;
        if (scales.ndim() == 2) {
            k_blocks = scales.size(1);
        } else if (scales.ndim() == 1) { // earlier versions of the spec used 1-D scales (contrib.rs:152-164)
            const int64_t k = lhs.ndim() >= 1 ? lhs.size(lhs.ndim() - 1) : 1;
            k_blocks = block_size > 0 ? k / block_size : 0;
            if (scales.len() != n * k_blocks) throw OpError(OpError::InvalidValue, "Expected 1D `scales` size to match columns * block_size");
        } else {
            throw OpError(OpError::InvalidValue, "Expected `scales` to have one or two dims");
        }
        if (in.size() > 3) throw OpError(OpError::UnsupportedValue, "zero_points, g_idx and bias inputs are unsupported");
        if (lhs.ndim() < 2) throw OpError(OpError::InvalidValue, "A input must have at least 2 dims");
        if (bits != 4 && bits != 8) throw OpError(OpError::UnsupportedValue, "Unsupported bits-per-element"); // BlockQuantizedMatrix::new (block_quant.rs:690-708)
        const int64_t elems_per_block = rhs.size(2) * (8 / bits);
        if (elems_per_block < 16 || (elems_per_block & (elems_per_block - 1))) throw OpError(OpError::UnsupportedValue, "Unsupported K block size");
        const int64_t rows = lhs.size(lhs.ndim() - 2), k = lhs.size(lhs.ndim() - 1);
        if (k != rhs.size(1) * elems_per_block) throw OpError(OpError::IncompatibleInputShapes, "Columns of first matrix does not match rows of second matrix");
        if (bits != 4) throw OpError(OpError::UnsupportedValue, "MatMulNBits: only 4-bit elements (GemmError::QuantBitsNotSupported, block_quant.rs:77-79)");
        if (scales.ndim() == 2 && (scales.size(0) != n || k_blocks != rhs.size(1))) throw OpError(OpError::IncompatibleInputShapes, "scales shape does not match the quantised matrix");
        std::vector<int64_t> out_shape(lhs.shape().begin(), lhs.shape().end() - 1);
        out_shape.push_back(n);
        int64_t batch = 1;
        for (int i = 0; i + 2 < lhs.ndim(); i++) batch *= lhs.size(i);
        Tensor y(ctx, out_shape, DType::F32);
        ctx.check(rten_hip_matmul_nbits_f32(ctx.raw(), batch, (int)rows, (int)k, (int)n, (int)elems_per_block, (const float *)lhs.ptr(), (const uint8_t *)rhs.ptr(),
                                            (const float *)scales.ptr(), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ row-wise / element-wise
inline int resolve_axis(int axis, int ndim) { // resolve_axis (src/ops/mod.rs): same message
    const int a = axis < 0 ? axis + ndim : axis;
    if (a < 0 || a >= ndim) throw OpError(OpError::InvalidValue, "Axis is invalid");
    return a;
}
// resolve_axes (src/ops/mod.rs:259-271): negative axes from the end, sorted, unique; none given = all
inline std::vector<int> resolve_axes(const std::vector<int> &axes, int nd) {
    std::vector<int> ax;
    if (axes.empty()) for (int d = 0; d < nd; d++) ax.push_back(d);
    for (int a : axes) ax.push_back(resolve_axis(a, nd));
    std::sort(ax.begin(), ax.end());
    ax.erase(std::unique(ax.begin(), ax.end()), ax.end());
    return ax;
}

struct Softmax : Operator { // src/ops/norm.rs:825-840 (last-axis lanes contiguous: other axes need a transpose first)
    int axis = -1;
    const char *name() const override { return "Softmax"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const int a = resolve_axis(axis, x.ndim());
        if (a != x.ndim() - 1) {
            // normalize_lanes (src/ops/norm.rs:705-754): move the axis last, make contiguous, apply, move it back
            const int nd = x.ndim();
            if (nd > 6) throw OpError(OpError::UnsupportedValue, "Softmax over a non-last axis of more than 6 dims is not supported by the device path");
            std::vector<int32_t> fwd, back((size_t)nd);
            for (int i = 0; i < nd; i++) if (i != a) fwd.push_back(i);
            fwd.push_back(a);
            for (int i = 0; i < nd; i++) back[(size_t)fwd[(size_t)i]] = i;
            std::vector<int64_t> tshape;
            for (int i = 0; i < nd; i++) tshape.push_back(x.size(fwd[(size_t)i]));
            Tensor t(ctx, tshape, DType::F32), u(ctx, tshape, DType::F32), y(ctx, x.shape(), DType::F32);
            if (x.len()) {
                const int64_t cols = x.size(a), rows = x.len() / cols;
                ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, x.shape().data(), fwd.data(), x.ptr(), t.ptr()));
                ctx.check(rten_hip_softmax_f32(ctx.raw(), rows, (int)cols, (const float *)t.ptr(), nullptr, 1, 1, 0, (float *)u.ptr()));
                ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, tshape.data(), back.data(), u.ptr(), y.ptr()));
            }
            OutputList out;
            out.push_back(std::move(y));
            return out;
        }
        const int64_t cols = x.size(a), rows = cols ? x.len() / cols : 0;
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(rten_hip_softmax_f32(ctx.raw(), rows, (int)cols, (const float *)x.ptr(), nullptr, 1, 1, 0, (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// LogSoftmax (src/ops/norm.rs:695-800 over rten-vecmath/src/softmax.rs:131-174): Softmax's route, any axis.
struct LogSoftmax : Operator {
    int axis = -1;
    const char *name() const override { return "LogSoftmax"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const int a = resolve_axis(axis, x.ndim());
        OutputList out;
        if (a != x.ndim() - 1) {
            const int nd = x.ndim();
            if (nd > 6) throw OpError(OpError::UnsupportedValue, "LogSoftmax over a non-last axis of more than 6 dims is not supported by the device path");
            std::vector<int32_t> fwd, back((size_t)nd);
            for (int i = 0; i < nd; i++) if (i != a) fwd.push_back(i);
            fwd.push_back(a);
            for (int i = 0; i < nd; i++) back[(size_t)fwd[(size_t)i]] = i;
            std::vector<int64_t> tshape;
            for (int i = 0; i < nd; i++) tshape.push_back(x.size(fwd[(size_t)i]));
            Tensor t(ctx, tshape, DType::F32), y(ctx, x.shape(), DType::F32);
            if (x.len()) {
                const int64_t cols = x.size(a), rows = x.len() / cols;
                ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, x.shape().data(), fwd.data(), x.ptr(), t.ptr()));
                ctx.check(rten_hip_log_softmax_f32(ctx.raw(), rows, (int)cols, (const float *)t.ptr(), (float *)t.ptr())); // in place: a wave stores a row after its last read of it
                ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, tshape.data(), back.data(), t.ptr(), y.ptr()));
            }
            out.push_back(std::move(y));
            return out;
        }
        const int64_t cols = x.size(a), rows = cols ? x.len() / cols : 0;
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(rten_hip_log_softmax_f32(ctx.raw(), rows, (int)cols, (const float *)x.ptr(), (float *)y.ptr()));
        out.push_back(std::move(y));
        return out;
    }
};

// BatchNormalization, inference form (src/ops/norm.rs:194-318): inputs X [N, C, ...] (a 1-D input has C = 1), scale, bias, mean, var [C].
// `act`: backend fusion of the following activation (the bits of the two operators in sequence).
struct BatchNormalization : Operator {
    float epsilon = 1e-5f;
    Activation act;
    const char *name() const override { return "BatchNormalization"; }
    int max_inputs() const override { return 5; }
    // the shape checks alone (the loader runs them on shapes): {n, channels, inner}
    static std::array<int64_t, 3> geometry(const std::vector<int64_t> &xs, int64_t scale0, int64_t bias0, int64_t mean0, int64_t var0) {
        if (xs.empty()) throw OpError(OpError::InvalidValue, "Input must have at least 1 dim");
        const int64_t channels = xs.size() >= 2 ? xs[1] : 1;
        if (scale0 != channels) throw OpError(OpError::IncompatibleInputShapes, "scale.size(0) != channels");
        if (bias0 != channels) throw OpError(OpError::IncompatibleInputShapes, "bias.size(0) != channels");
        if (mean0 != channels) throw OpError(OpError::IncompatibleInputShapes, "mean.size(0) != channels");
        if (var0 != channels) throw OpError(OpError::IncompatibleInputShapes, "var.size(0) != channels");
        const int64_t n = xs[0];
        return {n, channels, xs.size() >= 2 ? detail::prod(xs, 2, xs.size()) : 1};
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const Tensor *p[4];
        for (int i = 0; i < 4; i++) {
            p[i] = &want(require(in, (size_t)i + 1), DType::F32, "float32");
            if (p[i]->ndim() != 1) throw OpError(OpError::InvalidValue, "expected a vector"); // (NdTensorView<f32, 1> conversion)
        }
        const auto g = geometry(x.shape(), p[0]->size(0), p[1]->size(0), p[2]->size(0), p[3]->size(0));
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_batch_norm_f32_act(ctx.raw(), (int32_t)g[0], (int32_t)g[1], g[2], (const float *)x.ptr(), (const float *)p[0]->ptr(), (const float *)p[1]->ptr(),
                                                  (const float *)p[2]->ptr(), (const float *)p[3]->ptr(), epsilon, act.kind, act.alpha, act.beta, (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// InstanceNormalization (src/ops/norm.rs:320-395): inputs X [N, C, ...], scale [C], bias [C]; epsilon absent = 1e-5.  `act` as above.
struct InstanceNormalization : Operator {
    std::optional<float> epsilon;
    Activation act;
    const char *name() const override { return "InstanceNormalization"; }
    int max_inputs() const override { return 3; }
    static std::array<int64_t, 3> geometry(const std::vector<int64_t> &xs, int64_t scale0, int64_t bias0) {
        if (xs.size() < 2) throw OpError(OpError::InvalidValue, "expected input with >= 2 dims");
        if (scale0 != xs[1]) throw OpError(OpError::InvalidValue, "scale length should match channel count");
        if (bias0 != xs[1]) throw OpError(OpError::InvalidValue, "bias length should match channel count");
        return {xs[0], xs[1], detail::prod(xs, 2, xs.size())};
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const Tensor &scale = want(require(in, 1), DType::F32, "float32");
        const Tensor &bias = want(require(in, 2), DType::F32, "float32");
        if (scale.ndim() != 1 || bias.ndim() != 1) throw OpError(OpError::InvalidValue, "expected a vector");
        const auto g = geometry(x.shape(), scale.size(0), bias.size(0));
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_instance_norm_f32(ctx.raw(), (int32_t)g[0], (int32_t)g[1], g[2], (const float *)x.ptr(), (const float *)scale.ptr(), (const float *)bias.ptr(),
                                                 epsilon.value_or(1e-5f), act.kind, act.alpha, act.beta, (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

struct LayerNormalization : Operator { // src/ops/norm.rs:456-529
    int axis = -1;
    float epsilon = 1e-5f;
    const char *name() const override { return "LayerNormalization"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const Tensor &scale = want(require(in, 1), DType::F32, "float32");
        const Tensor *bias = get(in, 2);
        const int a = resolve_axis(axis, x.ndim());
        const int64_t cols = detail::prod(x.shape(), (size_t)a, x.shape().size()), rows = cols ? x.len() / cols : 0;
        if (scale.len() != cols) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast scale to input shape");
        if (bias && bias->len() != cols) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast bias to input shape");
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_layer_norm_f32(ctx.raw(), rows, (int)cols, (const float *)x.ptr(), (const float *)scale.ptr(), (const float *)vp(bias), 1.f, 0.f, epsilon,
                                              (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

template <int32_t (*FN)(rten_hip_ctx *, int64_t, const float *, float *)>
struct UnaryOp : Operator {
    const char *nm;
    explicit UnaryOp(const char *n) : nm(n) {}
    const char *name() const override { return nm; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(FN(ctx.raw(), x.len(), (const float *)x.ptr(), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};
struct Relu : UnaryOp<rten_hip_relu_f32> { Relu() : UnaryOp("Relu") {} };
struct Gelu : UnaryOp<rten_hip_gelu_f32> { Gelu() : UnaryOp("Gelu") {} };
struct Erf : UnaryOp<rten_hip_erf_f32> { Erf() : UnaryOp("Erf") {} };

// Sigmoid, Silu, Swish, HardSigmoid, HardSwish, LeakyRelu, Elu (rten-vecmath/src/exp.rs:201-275, relu.rs:13-25, src/ops/unary_elementwise.rs:437-471):
// one parameterised kernel, rten_hip_activation_f32
inline Tensor run_activation(Context &ctx, const Tensor &x, const Activation &a) {
    if (x.dtype() != DType::F32) throw OpError(OpError::UnsupportedType, "expected float32 tensor");
    Tensor y(ctx, x.shape(), DType::F32);
    if (x.len()) ctx.check(rten_hip_activation_f32(ctx.raw(), a.kind, a.alpha, a.beta, x.len(), (const float *)x.ptr(), (float *)y.ptr()));
    return y;
}
struct ActivationOp : Operator {
    Activation act;
    ActivationOp(int32_t kind, float alpha = 0.f, float beta = 0.f) { act.kind = kind; act.alpha = alpha; act.beta = beta; }
    const char *name() const override { return activation_name(act.kind); }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        OutputList out;
        out.push_back(run_activation(ctx, require(in, 0), act));
        return out;
    }
};
struct Sigmoid : ActivationOp { Sigmoid() : ActivationOp(RTEN_HIP_ACT_SIGMOID) {} };
struct Silu : ActivationOp { Silu() : ActivationOp(RTEN_HIP_ACT_SILU) {} };
struct Swish : ActivationOp { explicit Swish(float alpha = 1.f) : ActivationOp(RTEN_HIP_ACT_SWISH, alpha) {} };
struct HardSigmoid : ActivationOp { explicit HardSigmoid(float alpha = 0.2f, float beta = 0.5f) : ActivationOp(RTEN_HIP_ACT_HARD_SIGMOID, alpha, beta) {} };
struct HardSwish : ActivationOp { HardSwish() : ActivationOp(RTEN_HIP_ACT_HARD_SWISH) {} };
struct LeakyRelu : ActivationOp { explicit LeakyRelu(float alpha = 0.01f) : ActivationOp(RTEN_HIP_ACT_LEAKY_RELU, alpha) {} };
struct Elu : ActivationOp { explicit Elu(float alpha = 1.f) : ActivationOp(RTEN_HIP_ACT_ELU, alpha) {} };

// Clip(x, min?, max?) through the reference's Clamp trait (unary_elementwise.rs:248-303): a missing bound is f32::MIN / f32::MAX.
// f32 only; the bounds are scalars (read back to the host).
struct Clip : Operator {
    const char *name() const override { return "Clip"; }
    int max_inputs() const override { return 3; }
    static float bound(const Tensor *t, float dflt) {
        if (!t) return dflt;
        if (t->len() != 1) throw OpError(OpError::InvalidValue, "Clip: min / max must be scalars");
        if (t->dtype() != DType::F32) throw OpError(OpError::UnsupportedType, "Clip: expected float32 bounds");
        return t->to_host<float>()[0];
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        if (x.dtype() != DType::F32) throw OpError(OpError::UnsupportedType, "Clip: only float32 tensors are supported");
        Activation a;
        a.kind = RTEN_HIP_ACT_CLIP;
        a.alpha = bound(get(in, 1), -FLT_MAX);
        a.beta = bound(get(in, 2), FLT_MAX);
        OutputList out;
        out.push_back(run_activation(ctx, x, a));
        return out;
    }
};

template <int32_t (*FN)(rten_hip_ctx *, int64_t, const float *, const float *, int64_t, float *), int OPCODE>
struct BinaryOp : Operator { // binary_elementwise.rs:58-170,476-495: numpy broadcasting
    const char *nm;
    explicit BinaryOp(const char *n) : nm(n) {}
    const char *name() const override { return nm; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &a = want(require(in, 0), DType::F32, "float32"), &b = want(require(in, 1), DType::F32, "float32");
        const int64_t n = a.len(), bl = b.len();
        // fast path: equal shapes, or `b` broadcast over the leading dims of `a` (flat kernels, 16 B per lane)
        bool fast = bl > 0 && n % bl == 0 && b.ndim() <= a.ndim();
        for (int i = 0; fast && i < b.ndim(); i++) {
            const int64_t bd = b.size(b.ndim() - 1 - i), ad = a.size(a.ndim() - 1 - i);
            if (bd != ad && !(bd == 1 && detail::prod(b.shape(), 0, (size_t)(b.ndim() - 1 - i)) == 1)) fast = false;
        }
        OutputList out;
        if (fast) {
            Tensor y(ctx, a.shape(), DType::F32);
            if (n) ctx.check(FN(ctx.raw(), n, (const float *)a.ptr(), (const float *)b.ptr(), bl, (float *)y.ptr()));
            out.push_back(std::move(y));
            return out;
        }
        // general case: align the shapes on the right, stride 0 on every axis of extent 1
        const int nd = std::max(a.ndim(), b.ndim());
        if (nd > 6) throw OpError(OpError::UnsupportedValue, "broadcasting over more than 6 dims is not supported by the device path");
        std::vector<int64_t> oshape((size_t)nd), as((size_t)nd, 0), bs((size_t)nd, 0);
        int64_t sa = 1, sb = 1;
        for (int i = nd - 1; i >= 0; i--) {
            const int ia = i - (nd - a.ndim()), ib = i - (nd - b.ndim());
            const int64_t da = ia >= 0 ? a.size(ia) : 1, db = ib >= 0 ? b.size(ib) : 1;
            if (da != db && da != 1 && db != 1) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
            oshape[(size_t)i] = std::max(da, db) == 1 ? 1 : (da == 1 ? db : da);
            if (da == 0 || db == 0) oshape[(size_t)i] = 0;
            as[(size_t)i] = da == 1 ? 0 : sa;
            bs[(size_t)i] = db == 1 ? 0 : sb;
            sa *= da; sb *= db;
        }
        Tensor y(ctx, oshape, DType::F32);
        if (y.len()) ctx.check(rten_hip_binary_broadcast_f32(ctx.raw(), OPCODE, nd, oshape.data(), as.data(), bs.data(), (const float *)a.ptr(), (const float *)b.ptr(), (float *)y.ptr()));
        out.push_back(std::move(y));
        return out;
    }
};
struct Add : BinaryOp<rten_hip_add_f32, 0> { Add() : BinaryOp("Add") {} };
struct Mul : BinaryOp<rten_hip_mul_f32, 1> { Mul() : BinaryOp("Mul") {} };
struct Sub : BinaryOp<rten_hip_sub_f32, 2> { Sub() : BinaryOp("Sub") {} };
// Div (binary_elementwise.rs:613-637): a divisor of exactly ONE element, at any rank, is the reference's multiplication by the reciprocal -- a * (1 / b),
// two roundings, not a / b -- and every other divisor a true division.  (rten_hip_div_f32 and rten_hip_binary_broadcast_f32 op 3 stay true divisions.)
// The reciprocal of a divisor the host knows is uploaded once per context and value (by the warm-up run that precedes every capture) and the latest 8 are
// kept; a divisor may change from run to run (sum / Cast(Shape(x)[-1]) at changing shapes), and a reciprocal that a captured graph read stays where it is
// until that capture is destroyed (Context::retire).  A device scalar costs one RTEN_HIP_UNARY_RECIPROCAL launch on its element.  Both forms replay from a
// captured graph.
struct Div : BinaryOp<rten_hip_div_f32, 3> {
    Div() : BinaryOp("Div") {}
    OutputList run(Context &ctx, const InputList &in) const override {
        want(require(in, 0), DType::F32, "float32");
        const Tensor &b = want(require(in, 1), DType::F32, "float32");
        if (b.len() != 1) return BinaryOp::run(ctx, in);
        static const Mul mul;
        if (const HostVal *h = b.host()) {
            uint32_t bits;
            std::memcpy(&bits, &h->f.at(0), 4);
            std::lock_guard<std::mutex> lk(mu_);
            const Tensor *r = nullptr;
            for (const auto &e : reciprocals_) if (e.ctx == &ctx && e.bits == bits) r = e.value.get();
            if (!r) {
                if (rten_hip_capture_active(ctx.raw())) throw OpError(OpError::UnsupportedValue, "Div: the divisor's reciprocal must be uploaded before the run is captured");
                const float v = 1.0f / h->f[0];
                if (reciprocals_.size() >= 8) { // (the oldest goes; a captured graph that multiplies by it keeps its buffer: Context::retire)
                    reciprocals_.front().value->retire(reciprocals_.front().born);
                    reciprocals_.erase(reciprocals_.begin());
                }
                reciprocals_.push_back({&ctx, bits, ctx.stamp(), std::unique_ptr<Tensor>(new Tensor(Tensor::from_host_unpooled<float>(ctx, {}, &v)))});
                r = reciprocals_.back().value.get();
            }
            const Tensor rv = Tensor::view_of(*r, b.shape());
            return mul.run(ctx, {in[0], &rv});
        }
        Tensor r(ctx, b.shape(), DType::F32);
        ctx.check(rten_hip_unary_f32(ctx.raw(), RTEN_HIP_UNARY_RECIPROCAL, 1, (const float *)b.ptr(), (float *)r.ptr()));
        return mul.run(ctx, {in[0], &r});
    }
  private:
    struct Entry { const Context *ctx; uint32_t bits; uint64_t born; std::unique_ptr<Tensor> value; };
    mutable std::vector<Entry> reciprocals_;
    mutable std::mutex mu_;
};

// ------------------------------------------------------------------------------------------------ layout (src/ops/layout.rs, gather.rs)
struct Transpose : Operator { // layout.rs:669+: perm absent = reverse the axes
    std::vector<int> perm;
    const char *name() const override { return "Transpose"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        if (dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
        const int nd = x.ndim();
        std::vector<int32_t> p(perm.begin(), perm.end());
        if (p.empty()) for (int i = nd - 1; i >= 0; i--) p.push_back(i);
        if ((int)p.size() != nd) throw OpError(OpError::InvalidValue, "Permutation is invalid");
        std::vector<int64_t> oshape;
        for (int i = 0; i < nd; i++) {
            if (p[(size_t)i] < 0) p[(size_t)i] += nd;
            if (p[(size_t)i] < 0 || p[(size_t)i] >= nd) throw OpError(OpError::InvalidValue, "Permutation is invalid");
            oshape.push_back(x.size(p[(size_t)i]));
        }
        Tensor y(ctx, oshape, x.dtype());
        ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, x.shape().data(), p.data(), x.ptr(), y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// Gather (src/ops/gather.rs:21-110): 4-byte data, int32 indices, any axis; the embedding-lookup form (axis 0 of a float table) keeps its own kernel.
// Out-of-range indices are clamped on the device (the reference reports "Entry in `indices` is out of range").
struct Gather : Operator {
    int axis = 0;
    const char *name() const override { return "Gather"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &table = require(in, 0);
        const Tensor &ids = want(require(in, 1), DType::I32, "int32");
        if (dtype_size(table.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
        if (table.ndim() < 1) throw OpError(OpError::InvalidValue, "Input must have >= 1 dims");
        const int ax = resolve_axis(axis, table.ndim());
        std::vector<int64_t> oshape(table.shape().begin(), table.shape().begin() + ax);
        oshape.insert(oshape.end(), ids.shape().begin(), ids.shape().end());
        oshape.insert(oshape.end(), table.shape().begin() + ax + 1, table.shape().end());
        const int64_t outer = detail::prod(table.shape(), 0, (size_t)ax), inner = detail::prod(table.shape(), (size_t)ax + 1, table.shape().size());
        Tensor y(ctx, oshape, table.dtype());
        if (y.len()) {
            if (ax == 0 && table.dtype() == DType::F32)
                ctx.check(rten_hip_gather_rows_f32(ctx.raw(), ids.len(), (int32_t)inner, (int32_t)table.size(0), (const float *)table.ptr(), (const int32_t *)ids.ptr(), (float *)y.ptr()));
            else
                ctx.check(rten_hip_gather_axis_b32(ctx.raw(), outer, table.size(ax), inner, ids.len(), table.ptr(), (const int32_t *)ids.ptr(), y.ptr()));
        }
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// AddSoftmax (src/ops/attention.rs:94-156): softmax(x + m) over the last axis in one pass; m has x's shape, or is an
// attention mask [B, 1, 1, T] against x = [B, H, S, T], or a single row [T].
struct AddSoftmax : Operator {
    bool flush_nans_to_zero = false;
    const char *name() const override { return "AddSoftmax"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32"), &m = want(require(in, 1), DType::F32, "float32");
        if (x.ndim() < 1) throw OpError(OpError::InvalidValue, "Input must have >= 1 dims");
        const int64_t cols = x.size(x.ndim() - 1), rows = cols ? x.len() / cols : 0;
        int64_t add_div, add_mod;
        if (m.shape() == x.shape()) { add_div = 1; add_mod = rows ? rows : 1; }
        else if (m.len() == cols && m.size(m.ndim() - 1) == cols) { add_div = rows ? rows : 1; add_mod = 1; }
        else if (x.ndim() == 4 && m.ndim() == 4 && m.size(0) == x.size(0) && m.size(1) == 1 && m.size(2) == 1 && m.size(3) == cols) {
            add_div = x.size(1) * x.size(2); add_mod = x.size(0);
        } else throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(rten_hip_softmax_f32(ctx.raw(), rows, (int)cols, (const float *)x.ptr(), (const float *)m.ptr(), add_div, add_mod, flush_nans_to_zero ? 1 : 0, (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// Multi-head scaled dot-product attention over projection outputs laid out [B, S, heads * d] (head = column block): the
// Reshape / Transpose nodes around QK^T -> softmax -> PV become stride arithmetic (TransposeFusion's analogue,
// src/optimize/fusions.rs:1066; the core is sdpa_multi_head, src/ops/attention.rs:589-626).  Inputs q, k, v (+ additive mask
// [B,1,1,T] or [B,1,S,T]); q / k / v may be column blocks of one wider buffer: pass `row_stride` / `col_offset` views via
// the *_rs, *_off fields (elements).
struct MultiHeadSdpa : Operator {
    int heads = 1;
    int head_dim = 0; // heads <= 0: the graph's Reshape spells the head COUNT as -1 ([B, S, -1, d], transformers' exporter idiom): heads = hidden / head_dim
    float scale = 1.f;
    bool flush_nans_to_zero = false; // the FusedMatMul -> AddSoftmax -> MatMul graph does not flush; sdpa_head does (attention.rs:551)
    int64_t q_rs = 0, k_rs = 0, v_rs = 0;    // row strides (0: the tensor's own last dim)
    int64_t q_off = 0, k_off = 0, v_off = 0; // column offsets into the rows
    int64_t width = 0;                       // heads * d when q / k / v are column blocks of wider rows (0: last dim)
    const char *name() const override { return "MultiHeadSdpa"; }
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &q = want(require(in, 0), DType::F32, "float32"), &k = want(require(in, 1), DType::F32, "float32"), &v = want(require(in, 2), DType::F32, "float32");
        const Tensor *mask = get(in, 3);
        if (q.ndim() != 3 || k.ndim() != 3 || v.ndim() != 3) throw OpError(OpError::InvalidValue, "expected [batch, seq, hidden] projections");
        const int64_t B = q.size(0), S = q.size(1), T = k.size(1);
        const int64_t Hd = width ? width : q.size(2);
        const int heads = this->heads > 0 ? this->heads : (head_dim > 0 && Hd % head_dim == 0 ? (int)(Hd / head_dim) : 0);
        if (heads <= 0 || Hd % heads != 0) throw OpError(OpError::InvalidValue, "hidden size is not divisible by the number of heads");
        if (k.size(0) != B || v.size(0) != B || v.size(1) != T) throw OpError(OpError::IncompatibleInputShapes, "q / k / v batch or sequence sizes do not match");
        if (!width && (k.size(2) != Hd || v.size(2) != Hd)) throw OpError(OpError::IncompatibleInputShapes, "q / k / v hidden sizes do not match");
        const int64_t d = Hd / heads;
        rten_hip_sdpa_desc sd{};
        sd.batch = (int)B; sd.heads = heads; sd.s = (int)S; sd.t = (int)T; sd.d = (int)d; sd.dv = (int)d;
        sd.q_rs = q_rs ? q_rs : q.size(2); sd.k_rs = k_rs ? k_rs : k.size(2); sd.v_rs = v_rs ? v_rs : v.size(2);
        sd.q_bs = S * sd.q_rs; sd.k_bs = T * sd.k_rs; sd.v_bs = T * sd.v_rs;
        sd.q_hs = sd.k_hs = sd.v_hs = d;
        sd.o_rs = Hd; sd.o_bs = S * Hd; sd.o_hs = d;
        sd.scale = scale; sd.flush_nan_to_zero = flush_nans_to_zero ? 1 : 0;
        Tensor expanded; // a mask that broadcasts to [B, 1, S, T] in another form (e.g. a causal [1, 1, S, T] or [S, T]) is expanded first
        if (mask) {
            want(*mask, DType::F32, "float32");
            if (mask->ndim() == 4 && mask->size(0) == B && mask->size(1) == 1 && mask->size(3) == T && (mask->size(2) == 1 || mask->size(2) == S)) {
                // (an [B, 1, S, T] mask known to hold S copies of one row -- Tensor::uniform_dims, the exporter's expanded padding mask -- is read as that row)
                const bool one_row = mask->size(2) == 1 || (mask->uniform_dims() >> 2 & 1u);
                sd.mask_row_stride = one_row ? 0 : T;
                sd.mask_batch_stride = mask->size(2) == 1 ? T : S * T;
            } else {
                // numpy broadcasting of the Add(scores [B, H, S, T], mask): every form without a head axis is the same addend for
                // all heads, so the expanded copy gives the unfused graph's bits
                const int nd = mask->ndim();
                if (nd > 4) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
                int64_t ms[4] = {1, 1, 1, 1};
                for (int i = 0; i < nd; i++) ms[4 - nd + i] = mask->size(i);
                const int64_t want_shape[4] = {B, 1, S, T};
                if (ms[1] != 1) throw OpError(OpError::UnsupportedValue, "fused attention: a mask with a head axis is not supported (run the graph unfused)");
                int64_t strides[4], acc = 1;
                for (int i = 3; i >= 0; i--) {
                    if (ms[i] != 1 && ms[i] != want_shape[i]) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
                    strides[i] = ms[i] == 1 ? 0 : acc;
                    acc *= ms[i];
                }
                expanded = Tensor(ctx, {B, 1, S, T}, DType::F32);
                if (expanded.len()) ctx.check(rten_hip_copy_strided_b32(ctx.raw(), 4, want_shape, strides, mask->ptr(), expanded.ptr()));
                mask = &expanded;
                sd.mask_row_stride = T;
                sd.mask_batch_stride = S * T;
            }
        }
        Tensor y(ctx, {B, S, Hd}, DType::F32);
        if (y.len())
            ctx.check(rten_hip_sdpa_f32(ctx.raw(), &sd, (const float *)q.ptr() + q_off, (const float *)k.ptr() + k_off, (const float *)v.ptr() + v_off,
                                        (const float *)vp(mask), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// Add(residual) -> LayerNormalization as one kernel (the sum is formed in registers in the reference's order: x + r).
struct AddLayerNormalization : Operator {
    float epsilon = 1e-5f;
    const char *name() const override { return "AddLayerNormalization"; }
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32"), &r = want(require(in, 1), DType::F32, "float32");
        const Tensor &scale = want(require(in, 2), DType::F32, "float32");
        const Tensor *bias = get(in, 3);
        if (x.shape() != r.shape()) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
        const int64_t cols = x.ndim() ? x.size(x.ndim() - 1) : 1, rows = cols ? x.len() / cols : 0;
        if (scale.len() != cols) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast scale to input shape");
        if (bias && bias->len() != cols) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast bias to input shape");
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_add_layer_norm_f32(ctx.raw(), rows, (int)cols, (const float *)x.ptr(), (const float *)r.ptr(), (const float *)scale.ptr(), (const float *)vp(bias), 1.f,
                                                  0.f, epsilon, (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ pooling
struct PoolBase : Operator {
    std::vector<int> kernel_size{1, 1}, strides{1, 1};
    Padding padding;
    bool ceil_mode = false;
    rten_hip_pool2d_desc desc(const Tensor &x, bool count_include_pad) const {
        if (x.ndim() != 4) throw OpError(OpError::InvalidValue, "input must have 4 dims (NCHW)");
        const OutputSize os = calc_output_size_and_padding((int)x.size(2), (int)x.size(3), kernel_size[0], kernel_size[1], strides, padding, {1, 1}, ceil_mode);
        rten_hip_pool2d_desc d{};
        d.n = (int)x.size(0); d.c = (int)x.size(1); d.h = (int)x.size(2); d.w = (int)x.size(3);
        d.kh = kernel_size[0]; d.kw = kernel_size[1]; d.stride_h = strides[0]; d.stride_w = strides[1];
        for (int i = 0; i < 4; i++) d.pads[i] = os.pads[i];
        d.out_h = os.oh; d.out_w = os.ow; d.count_include_pad = count_include_pad;
        return d;
    }
};
struct MaxPool : PoolBase { // src/ops/pooling.rs:477-521
    void *stats_out = nullptr; // executor-set: a DynamicQuantizeLinear reads the output next -> its min / max come out of this launch
    const char *name() const override { return "MaxPool"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const rten_hip_pool2d_desc d = desc(x, false);
        Tensor y(ctx, {d.n, d.c, d.out_h, d.out_w}, DType::F32);
        if (stats_out) ctx.check(rten_hip_max_pool2d_f32_stats(ctx.raw(), &d, (const float *)x.ptr(), (float *)y.ptr(), stats_out));
        else ctx.check(rten_hip_max_pool2d_f32(ctx.raw(), &d, (const float *)x.ptr(), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};
struct AveragePool : PoolBase { // src/ops/pooling.rs:174-389
    bool count_include_pad = false;
    const char *name() const override { return "AveragePool"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const rten_hip_pool2d_desc d = desc(x, count_include_pad);
        Tensor y(ctx, {d.n, d.c, d.out_h, d.out_w}, DType::F32);
        ctx.check(rten_hip_average_pool2d_f32(ctx.raw(), &d, (const float *)x.ptr(), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};
struct GlobalAveragePool : Operator { // src/ops/pooling.rs:392-417
    const char *name() const override { return "GlobalAveragePool"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        if (x.ndim() != 4) throw OpError(OpError::InvalidValue, "input must have 4 dims (NCHW)");
        Tensor y(ctx, {x.size(0), x.size(1), 1, 1}, DType::F32);
        if (x.len()) ctx.check(rten_hip_global_average_pool_f32(ctx.raw(), x.size(0) * x.size(1), (int)(x.size(2) * x.size(3)), (const float *)x.ptr(), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ quantization
struct DynamicQuantizeLinear : Operator { // src/ops/quantize.rs:352-436: outputs y (u8), y_scale (f32 scalar), y_zero_point (u8 scalar)
    const char *name() const override { return "DynamicQuantizeLinear"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        Tensor y(ctx, x.shape(), DType::U8), s(ctx, {}, DType::F32), z(ctx, {}, DType::U8);
        ctx.check(rten_hip_dynamic_quantize_linear(ctx.raw(), x.len(), (const float *)x.ptr(), (uint8_t *)y.ptr(), (float *)s.ptr(), (uint8_t *)z.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        out.push_back(std::move(s));
        out.push_back(std::move(z));
        return out;
    }
};

// QuantizeLinear / DequantizeLinear (src/ops/quantize.rs:41-334).  qdq_geometry: the reference's rules on the shapes -> [outer][channels][inner].  A scalar or
// one-element scale is per-tensor (its zero point must have one element), a rank-1 scale per-axis (checked against the axis), anything else blocked
// quantisation.  One deviation: the reference does not check the zero-point length of a per-axis QuantizeLinear (its zip is cut short); a mismatch is refused
// with DequantizeLinear's message.  `zp_shape` null = no zero point.
struct QdqGeometry { int64_t outer = 1, channels = 1, inner = 1; int axis = -1; }; // axis: the resolved axis of a per-axis form, -1 per-tensor
inline int64_t shape_len(const std::vector<int64_t> &s) { int64_t n = 1; for (int64_t d : s) n *= d; return n; }
inline QdqGeometry qdq_geometry(const std::vector<int64_t> &x, const std::vector<int64_t> &scale, const std::vector<int64_t> *zp_shape, int axis, bool dequantize) {
    QdqGeometry g;
    if (shape_len(scale) == 1) {
        if (zp_shape && shape_len(*zp_shape) != 1) throw OpError(OpError::InvalidValue, "scale and zero_point must have same shape");
        g.inner = shape_len(x);
        return g;
    }
    if (scale.size() != 1) throw OpError(OpError::UnsupportedValue, dequantize ? "Blocked dequantization is not supported" : "Blocked quantization is not supported");
    const int ax = resolve_axis(axis, (int)x.size());
    if (scale[0] != x[(size_t)ax]) throw OpError(OpError::IncompatibleInputShapes, "scale length does not match size of quantization axis");
    if (zp_shape) {
        if (zp_shape->size() != 1) throw OpError(OpError::InvalidValue, dequantize ? "scale and zero point must have same rank" : "scale and zero point must have same shape");
        if ((*zp_shape)[0] != x[(size_t)ax]) throw OpError(OpError::IncompatibleInputShapes, "zero_point length does not match size of quantization axis");
    }
    g.axis = ax;
    g.channels = x[(size_t)ax];
    for (int d = 0; d < ax; d++) g.outer *= x[(size_t)d];
    for (size_t d = (size_t)ax + 1; d < x.size(); d++) g.inner *= x[d];
    return g;
}
inline int qdq_dtype_code(DType t) { return t == DType::U8 ? RTEN_HIP_DT_U8 : t == DType::I8 ? RTEN_HIP_DT_I8 : t == DType::I32 ? RTEN_HIP_DT_I32 : -1; }

struct QuantizeLinear : Operator {
    int axis = -1;
    std::optional<DType> output_dtype; // U8 / I8; used when there is no zero point
    const char *name() const override { return "QuantizeLinear"; }
    int max_inputs() const override { return 3; }
    // quantize.rs:299-323: the zero point's type (which output_dtype, if given, must equal), or output_dtype alone
    DType out_dtype(const Tensor *zp) const {
        if (zp) {
            if ((zp->dtype() == DType::U8 || zp->dtype() == DType::I8) && (!output_dtype || *output_dtype == zp->dtype())) return zp->dtype();
        } else if (output_dtype && (*output_dtype == DType::U8 || *output_dtype == DType::I8)) return *output_dtype;
        throw OpError(OpError::UnsupportedType, "");
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32"), &scale = want(require(in, 1), DType::F32, "float32");
        const Tensor *zp = get(in, 2);
        const DType dt = out_dtype(zp);
        const QdqGeometry g = qdq_geometry(x.shape(), scale.shape(), zp ? &zp->shape() : nullptr, axis, false);
        Tensor y(ctx, x.shape(), dt);
        if (x.len()) ctx.check(rten_hip_quantize_linear_f32(ctx.raw(), qdq_dtype_code(dt), g.outer, g.channels, g.inner, (const float *)x.ptr(), (const float *)scale.ptr(), vp(zp), y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

struct DequantizeLinear : Operator {
    int axis = 1;
    const char *name() const override { return "DequantizeLinear"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0), &scale = want(require(in, 1), DType::F32, "float32");
        if (qdq_dtype_code(x.dtype()) < 0) throw OpError(OpError::UnsupportedType, "");
        const Tensor *zp = get(in, 2);
        if (zp) want(*zp, x.dtype(), x.dtype() == DType::U8 ? "uint8" : x.dtype() == DType::I8 ? "int8" : "int32");
        const QdqGeometry g = qdq_geometry(x.shape(), scale.shape(), zp ? &zp->shape() : nullptr, axis, true);
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(rten_hip_dequantize_linear_f32(ctx.raw(), qdq_dtype_code(x.dtype()), g.outer, g.channels, g.inner, x.ptr(), (const float *)scale.ptr(), vp(zp), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// QuantizeLinear -> DequantizeLinear with equal parameters as one pass (the graph executor's pair fusion): f32 -> f32, the bits of the two operators run back
// to back.  Inputs as QuantizeLinear's.
struct QuantizeDequantizeLinear : Operator {
    QuantizeLinear q;
    const char *name() const override { return "QuantizeLinear+DequantizeLinear"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32"), &scale = want(require(in, 1), DType::F32, "float32");
        const Tensor *zp = get(in, 2);
        const DType dt = q.out_dtype(zp);
        const QdqGeometry g = qdq_geometry(x.shape(), scale.shape(), zp ? &zp->shape() : nullptr, q.axis, false);
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(rten_hip_quantize_dequantize_f32(ctx.raw(), qdq_dtype_code(dt), g.outer, g.channels, g.inner, (const float *)x.ptr(), (const float *)scale.ptr(), vp(zp), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// DynamicQuantizeLinear whose u8 output is only consumed by int8 convolutions of one staging geometry: the codes are
// written once, directly in the kernel's staged layout (bit-identical values), and -- when the producer of `x` left
// min/max statistics -- without the extra sweep over x.  Outputs: staged image (logical shape of x), y_scale, y_zero_point.
struct DynamicQuantizeLinearStaged : Operator {
    ConvInteger consumer;        // geometry attributes of (one of) the consuming convolutions
    std::vector<int64_t> kernel; // [O, C/g, kh, kw] of that consumer
    const void *stats_in = nullptr;
    // optional: the scalar Mul(y_scale, w_scale) nodes that follow in ort-quantized graphs, one per convolution reading the codes (a stage's
    // shortcut and first 1x1 share one quantizer) -> outputs 4, 5, ... in this order (rten_hip_dynamic_quantize_linear_staged_products)
    std::vector<const Tensor *> mul_by;
    static constexpr size_t kMaxProducts = 4;
    const char *name() const override { return "DynamicQuantizeLinear"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        rten_hip_conv2d_int8_desc di{};
        di.conv = consumer.conv.geometry(x.shape(), kernel);
        di.x_signed = 0; di.w_signed = 1; di.pad_mode = consumer.pad_mode;
        const size_t nbytes = rten_hip_conv2d_int8_staged_bytes(&di);
        if (!nbytes) throw OpError(OpError::UnsupportedValue, "quantize_staged: geometry not covered by the staged kernel");
        if (mul_by.size() > kMaxProducts) throw OpError(OpError::UnsupportedValue, "quantize_staged: at most 4 scale products per launch");
        Tensor y(ctx, x.shape(), DType::U8, nbytes), s(ctx, {}, DType::F32), z(ctx, {}, DType::U8);
        std::vector<Tensor> prods;
        prods.reserve(kMaxProducts);
        const float *mb[kMaxProducts] = {};
        float *pr[kMaxProducts] = {};
        for (size_t i = 0; i < mul_by.size(); i++) {
            if (!mul_by[i] || mul_by[i]->len() != 1) throw OpError(OpError::InvalidValue, "scale should be a scalar");
            prods.emplace_back(ctx, mul_by[i]->shape(), DType::F32);
            mb[i] = (const float *)mul_by[i]->ptr();
            pr[i] = (float *)prods.back().ptr();
        }
        ctx.check(rten_hip_dynamic_quantize_linear_staged_products(ctx.raw(), &di, (const float *)x.ptr(), stats_in, y.ptr(), (float *)s.ptr(), (uint8_t *)z.ptr(),
                                                                   (int32_t)mul_by.size(), mul_by.empty() ? nullptr : mb, mul_by.empty() ? nullptr : pr));
        OutputList out;
        out.push_back(std::move(y));
        out.push_back(std::move(s));
        out.push_back(std::move(z));
        for (Tensor &t : prods) out.push_back(std::move(t));
        return out;
    }

    // This quantizer INSIDE the launch of the ConvIntegerToFloat step `prod` that produces its input (rten_hip_conv2d_int8_qout: the f32 values never
    // leave the registers unless `keep_f32` -- a residual Add also reads them).  `in` = prod's X (staged), W, x_zp, w_zp; `sync` = the edge's exchange
    // block.  out = {prod's f32 output (empty unless keep_f32), codes, scale, zero point[, product]}.  Returns false when the launch form does not
    // apply (geometry not covered, or more workgroups than the device holds at once: RTEN_HIP_ERR_UNSUPPORTED): run the two operators then.  Opt-in
    // (launch plan) only: see the time-out contract in rten_hip.h.
    // `sync` == nullptr with `recompute`: the two-launch recompute form (statistics-only pass, then the convolution again with the codes as its output) -- no
    // grid-wide exchange, so replicas running side by side may use it.
    bool run_in_producer(Context &ctx, const ConvInteger &prod, const InputList &in, const Tensor &scale, const Tensor *bias, const Tensor *residual, bool relu,
                         const ConvInteger::Staging &sg, bool per_channel_scale, void *sync, bool keep_f32, OutputList &out, bool recompute = false) const {
        if (mul_by.size() > kMaxProducts || (!sync && !recompute) || !sg.stats_out || !sg.x_staged || !sg.packed_weight || !sg.packed_weight->len()) return false;
        if (recompute) sync = nullptr;
        const Tensor &x = require(in, 0), &w = require(in, 1);
        const Tensor *x_zp = get(in, 2), *w_zp = get(in, 3);
        rten_hip_conv2d_int8_desc di = prod.desc(x, w, x_zp, w_zp);
        di.weights_packed = 1;
        di.x_staged = 1;
        if (per_channel_scale) di.scale_len = di.conv.o;
        const std::vector<int64_t> yshape{di.conv.n, di.conv.o, di.conv.out_h, di.conv.out_w};
        rten_hip_conv2d_int8_desc dn{};
        dn.conv = consumer.conv.geometry(yshape, kernel);
        dn.x_signed = 0; dn.w_signed = 1; dn.pad_mode = consumer.pad_mode;
        const size_t nbytes = rten_hip_conv2d_int8_staged_bytes(&dn);
        if (!nbytes) return false;
        for (const Tensor *mb : mul_by) if (!mb || mb->len() != 1) throw OpError(OpError::InvalidValue, "scale should be a scalar");
        Tensor y(ctx, keep_f32 ? yshape : std::vector<int64_t>{0}, DType::F32);
        Tensor q(ctx, yshape, DType::U8, nbytes), s(ctx, {}, DType::F32), z(ctx, {}, DType::U8);
        Tensor pr(ctx, mul_by.empty() ? std::vector<int64_t>{0} : mul_by[0]->shape(), DType::F32);
        const uint32_t flags = (relu ? RTEN_HIP_CONV_RELU : 0u) | (residual ? RTEN_HIP_CONV_RESIDUAL : 0u);
        const int32_t rc = rten_hip_conv2d_int8_qout(ctx.raw(), &di, x.ptr(), sg.packed_weight->ptr(), vp(x_zp), vp(w_zp), (const float *)scale.ptr(),
                                                     (const float *)vp(bias), (const float *)vp(residual), flags, keep_f32 ? (float *)y.ptr() : nullptr, sg.stats_out, sync,
                                                     &dn, q.ptr(), (float *)s.ptr(), (uint8_t *)z.ptr(), mul_by.empty() ? nullptr : (const float *)mul_by[0]->ptr(),
                                                     mul_by.empty() ? nullptr : (float *)pr.ptr());
        if (rc == RTEN_HIP_ERR_UNSUPPORTED) return false;
        ctx.check(rc);
        // a quantizer read by several convolutions (a stage's shortcut and first 1x1): the launch folds the first Mul(y_scale, w_scale); the others
        // are the graph's own scalar Mul nodes, one tiny launch each (same f32 multiply)
        std::vector<Tensor> more;
        for (size_t i = 1; i < mul_by.size(); i++) {
            more.emplace_back(ctx, mul_by[i]->shape(), DType::F32);
            ctx.check(rten_hip_mul_f32(ctx.raw(), 1, (const float *)s.ptr(), (const float *)mul_by[i]->ptr(), 1, (float *)more.back().ptr()));
        }
        out.clear();
        out.push_back(std::move(y));
        out.push_back(std::move(q));
        out.push_back(std::move(s));
        out.push_back(std::move(z));
        if (!mul_by.empty()) out.push_back(std::move(pr));
        for (Tensor &t : more) out.push_back(std::move(t));
        return true;
    }
};

// Cast (src/ops/convert.rs): the device path covers what the quantized graphs need, int32 -> float32 (exact conversion with
// round-to-nearest-even above 2^24, the same instruction cast_scale uses) and identity casts.
inline int32_t abi_dtype(DType t) { return t == DType::F32 ? RTEN_HIP_DT_F32 : t == DType::I32 ? RTEN_HIP_DT_I32 : t == DType::U8 ? RTEN_HIP_DT_U8 : RTEN_HIP_DT_I8; }

// numpy broadcasting of up to three operands: the common shape and each operand's element strides on it (0 on broadcast axes)
struct Broadcast {
    std::vector<int64_t> shape;
    std::vector<int64_t> strides[3];
};
inline Broadcast broadcast_shapes(const std::vector<const std::vector<int64_t> *> &shapes) {
    Broadcast b;
    size_t nd = 0;
    for (auto *sh : shapes) nd = std::max(nd, sh->size());
    if (nd > 6) throw OpError(OpError::UnsupportedValue, "broadcasting over more than 6 dims is not supported by the device path");
    b.shape.assign(nd, 1);
    for (auto *sh : shapes)
        for (size_t i = 0; i < sh->size(); i++) {
            const size_t o = nd - sh->size() + i;
            const int64_t d = (*sh)[i];
            if (d != 1) {
                if (b.shape[o] != 1 && b.shape[o] != d) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
                b.shape[o] = d;
            }
        }
    for (size_t k = 0; k < shapes.size() && k < 3; k++) {
        const auto &sh = *shapes[k];
        b.strides[k].assign(nd, 0);
        int64_t acc = 1;
        for (size_t i = sh.size(); i-- > 0;) {
            b.strides[k][nd - sh.size() + i] = sh[i] == 1 ? 0 : acc;
            acc *= sh[i];
        }
    }
    return b;
}

// Which dims of an element-wise result are uniform (Tensor::uniform_dims): dim d of the broadcast shape is, when EVERY operand is constant along it -- its own
// size there is 1 (or the dim is absent), it carries the flag, or it is a host value whose slices along that dim are equal (checked here, the values are small).
inline bool host_uniform_along(const HostVal &h, size_t dim) {
    int64_t inner = 1, n = h.shape[dim];
    for (size_t i = dim + 1; i < h.shape.size(); i++) inner *= h.shape[i];
    const int64_t total = h.len();
    if (n <= 1 || total == 0) return true;
    for (int64_t base = 0; base < total; base += n * inner)
        for (int64_t k = 1; k < n; k++)
            for (int64_t j = 0; j < inner; j++) {
                const size_t x = (size_t)(base + j), y = (size_t)(base + k * inner + j);
                if (h.is_float ? std::memcmp(&h.f[x], &h.f[y], 4) != 0 : h.i[x] != h.i[y]) return false;
            }
    return true;
}
inline uint32_t uniform_after_broadcast(const std::vector<const Tensor *> &ins, const std::vector<int64_t> &out_shape) {
    uint32_t m = 0;
    const size_t nd = out_shape.size();
    for (size_t d = 0; d < nd && d < 32; d++) {
        if (out_shape[d] <= 1) continue; // (a size-1 dim carries no information; consumers test sizes first)
        bool all = true;
        for (const Tensor *t : ins) {
            if (!t) continue;
            const size_t tn = (size_t)t->ndim();
            if (d + tn < nd) continue;               // the operand has no such dim: broadcast along it
            const size_t td = d - (nd - tn);
            if (t->size((int)td) == 1) continue;
            if (t->uniform_dims() >> td & 1u) continue;
            if (t->host() && t->host()->len() <= (int64_t)1 << 20 && host_uniform_along(*t->host(), td)) continue;
            all = false;
            break;
        }
        if (all) m |= 1u << d;
    }
    return m;
}

struct Cast : Operator { // src/ops/convert.rs:18-60: every pair of float32 / int32 / uint8 / int8 (`as` casts)
    DType to = DType::F32;
    const char *name() const override { return "Cast"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        OutputList out;
        Tensor y(ctx, x.shape(), to);
        if (x.dtype() == to) { // identity cast: a copy
            if (x.bytes()) ctx.check(rten_hip_memcpy_d2d(ctx.raw(), y.ptr(), x.ptr(), x.bytes()));
        } else if (x.dtype() == DType::I32 && to == DType::F32) {
            if (x.len()) ctx.check(rten_hip_cast_scale(ctx.raw(), x.len(), (const int32_t *)x.ptr(), ctx.one(), 1, (float *)y.ptr()));
        } else if (x.len()) {
            const int64_t n = x.len(), one = 1;
            ctx.check(rten_hip_elementwise_nd(ctx.raw(), RTEN_HIP_EW_CAST, 1, &n, x.ptr(), abi_dtype(x.dtype()), &one, nullptr, 0, nullptr, nullptr, nullptr, y.ptr(), abi_dtype(to)));
        }
        y.set_uniform_dims(x.uniform_dims());
        out.push_back(std::move(y));
        return out;
    }
};

struct Tanh : UnaryOp<rten_hip_tanh_f32> { Tanh() : UnaryOp("Tanh") {} }; // rten-vecmath/src/tanh.rs (BERT's pooler)

// Not / And / Or / Xor, Equal / Less / LessOrEqual / Greater / GreaterOrEqual, integer Add / Sub / Mul / Div: numpy broadcasting, int32 results
// (unary_elementwise.rs:563-565, binary_elementwise.rs:546-598,733-786).  `code` = the RTEN_HIP_EW_* operation.
struct ElementwiseNd : Operator {
    int code = RTEN_HIP_EW_AND;
    const char *nm = "And";
    ElementwiseNd() = default;
    ElementwiseNd(int c, const char *n) : code(c), nm(n) {}
    const char *name() const override { return nm; }
    int max_inputs() const override { return code == RTEN_HIP_EW_NOT ? 1 : 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &a = require(in, 0);
        OutputList out;
        if (code == RTEN_HIP_EW_NOT) {
            want(a, DType::I32, "int32");
            Tensor y(ctx, a.shape(), DType::I32);
            const int64_t n = a.len(), one = 1;
            if (n) ctx.check(rten_hip_elementwise_nd(ctx.raw(), code, 1, &n, a.ptr(), RTEN_HIP_DT_I32, &one, nullptr, 0, nullptr, nullptr, nullptr, y.ptr(), RTEN_HIP_DT_I32));
            y.set_uniform_dims(a.uniform_dims());
            out.push_back(std::move(y));
            return out;
        }
        const Tensor &b = require(in, 1);
        const bool cmp = code >= RTEN_HIP_EW_EQUAL && code <= RTEN_HIP_EW_GREATER_EQ;
        if (cmp) { if (a.dtype() != b.dtype() || (a.dtype() != DType::F32 && a.dtype() != DType::I32)) throw OpError(OpError::UnsupportedType, ""); }
        else { want(a, DType::I32, "int32"); want(b, DType::I32, "int32"); }
        const Broadcast bc = broadcast_shapes({&a.shape(), &b.shape()});
        Tensor y(ctx, bc.shape, DType::I32);
        if (y.len())
            ctx.check(rten_hip_elementwise_nd(ctx.raw(), code, (int32_t)bc.shape.size(), bc.shape.data(), a.ptr(), abi_dtype(a.dtype()), bc.strides[0].data(), b.ptr(), abi_dtype(b.dtype()),
                                              bc.strides[1].data(), nullptr, nullptr, y.ptr(), RTEN_HIP_DT_I32));
        y.set_uniform_dims(uniform_after_broadcast({&a, &b}, bc.shape));
        out.push_back(std::move(y));
        return out;
    }
};

struct Where : Operator { // binary_elementwise.rs:1189-1280: cond != 0 ? x : y, the three operands broadcast together
    const char *name() const override { return "Where"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &c = want(require(in, 0), DType::I32, "int32"), &x = require(in, 1), &y = require(in, 2);
        if (x.dtype() != y.dtype() || dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
        const Broadcast bc = broadcast_shapes({&c.shape(), &x.shape(), &y.shape()});
        Tensor o(ctx, bc.shape, x.dtype());
        if (o.len())
            ctx.check(rten_hip_elementwise_nd(ctx.raw(), RTEN_HIP_EW_WHERE, (int32_t)bc.shape.size(), bc.shape.data(), c.ptr(), RTEN_HIP_DT_I32, bc.strides[0].data(), x.ptr(),
                                              abi_dtype(x.dtype()), bc.strides[1].data(), y.ptr(), bc.strides[2].data(), o.ptr(), abi_dtype(x.dtype())));
        o.set_uniform_dims(uniform_after_broadcast({&c, &x, &y}, bc.shape));
        OutputList out;
        out.push_back(std::move(o));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ unary math, Pow, PRelu, variadic Min / Max / Sum / Mean, Pad
// Neg, Abs, Sign, Floor, Ceil, Round, Sqrt, Reciprocal, Exp, Log, Softplus (src/ops/unary_elementwise.rs): float32 through rten_hip_unary_f32 (`code`, one kernel
// instantiation per operator); the operators the reference also defines for int32 (Neg, Abs, Sign) through `int_code` of rten_hip_elementwise_nd.
struct UnaryMath : Operator {
    const char *nm;
    int code, int_code;
    UnaryMath(const char *n, int c, int ic = -1) : nm(n), code(c), int_code(ic) {}
    const char *name() const override { return nm; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        OutputList out;
        if (int_code >= 0 && x.dtype() == DType::I32) {
            Tensor y(ctx, x.shape(), DType::I32);
            const int64_t n = x.len(), one = 1;
            if (n) ctx.check(rten_hip_elementwise_nd(ctx.raw(), int_code, 1, &n, x.ptr(), RTEN_HIP_DT_I32, &one, nullptr, 0, nullptr, nullptr, nullptr, y.ptr(), RTEN_HIP_DT_I32));
            y.set_uniform_dims(x.uniform_dims());
            out.push_back(std::move(y));
            return out;
        }
        if (int_code >= 0 && x.dtype() != DType::F32) throw OpError(OpError::UnsupportedType, "");
        want(x, DType::F32, "float32");
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) ctx.check(rten_hip_unary_f32(ctx.raw(), code, x.len(), (const float *)x.ptr(), (float *)y.ptr()));
        y.set_uniform_dims(x.uniform_dims());
        out.push_back(std::move(y));
        return out;
    }
};
struct Neg : UnaryMath { Neg() : UnaryMath("Neg", RTEN_HIP_UNARY_NEG, RTEN_HIP_EW_INEG) {} };
struct Abs : UnaryMath { Abs() : UnaryMath("Abs", RTEN_HIP_UNARY_ABS, RTEN_HIP_EW_IABS) {} };
struct Sign : UnaryMath { Sign() : UnaryMath("Sign", RTEN_HIP_UNARY_SIGN, RTEN_HIP_EW_ISIGN) {} }; // Rust signum: +0 -> 1, -0 -> -1, NaN -> NaN
struct Floor : UnaryMath { Floor() : UnaryMath("Floor", RTEN_HIP_UNARY_FLOOR) {} };
struct Ceil : UnaryMath { Ceil() : UnaryMath("Ceil", RTEN_HIP_UNARY_CEIL) {} };
struct Round : UnaryMath { Round() : UnaryMath("Round", RTEN_HIP_UNARY_ROUND) {} }; // round_ties_even
struct Sqrt : UnaryMath { Sqrt() : UnaryMath("Sqrt", RTEN_HIP_UNARY_SQRT) {} };
struct Reciprocal : UnaryMath { Reciprocal() : UnaryMath("Reciprocal", RTEN_HIP_UNARY_RECIPROCAL) {} };
struct Exp : UnaryMath { Exp() : UnaryMath("Exp", RTEN_HIP_UNARY_EXP) {} };
struct Log : UnaryMath { Log() : UnaryMath("Log", RTEN_HIP_UNARY_LOG) {} };                // the float64 logarithm rounded once (docs/KERNELS.md 4.8)
struct Softplus : UnaryMath { Softplus() : UnaryMath("Softplus", RTEN_HIP_UNARY_SOFTPLUS) {} };

// y = op(a, b) with numpy broadcasting and the operand order kept: float32 through rten_hip_binary_broadcast_f32 (`f32_op`), int32 through
// rten_hip_elementwise_nd (`i32_op`); both operands have the same 4-byte type
inline Tensor broadcast_binary(Context &ctx, const Tensor &a, const Tensor &b, int f32_op, int i32_op) {
    const Broadcast bc = broadcast_shapes({&a.shape(), &b.shape()});
    Tensor y(ctx, bc.shape, a.dtype());
    if (y.len()) {
        if (a.dtype() == DType::F32)
            ctx.check(rten_hip_binary_broadcast_f32(ctx.raw(), f32_op, (int32_t)bc.shape.size(), bc.shape.data(), bc.strides[0].data(), bc.strides[1].data(), (const float *)a.ptr(),
                                                    (const float *)b.ptr(), (float *)y.ptr()));
        else
            ctx.check(rten_hip_elementwise_nd(ctx.raw(), i32_op, (int32_t)bc.shape.size(), bc.shape.data(), a.ptr(), RTEN_HIP_DT_I32, bc.strides[0].data(), b.ptr(), RTEN_HIP_DT_I32,
                                              bc.strides[1].data(), nullptr, nullptr, y.ptr(), RTEN_HIP_DT_I32));
    }
    y.set_uniform_dims(uniform_after_broadcast({&a, &b}, bc.shape));
    return y;
}

// Pow (src/ops/binary_elementwise.rs:958-1117), float32 base and exponent: exponent 2 -> x * x, 3 -> x * x * x, tested per element; anything else the float64
// pow rounded once.  The reference's int32-base forms are not built.
struct Pow : Operator {
    const char *name() const override { return "Pow"; }
    int max_inputs() const override { return 2; }
    static void check_types(DType base, DType exponent) {
        if (base == DType::I32 && (exponent == DType::F32 || exponent == DType::I32)) throw OpError(OpError::UnsupportedValue, "Pow: int32 base is not supported by the device path");
        if (base != DType::F32 || exponent != DType::F32) throw OpError(OpError::UnsupportedValue, "Unsupported base and exponent type combination");
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &base = require(in, 0), &exponent = require(in, 1);
        check_types(base.dtype(), exponent.dtype());
        OutputList out;
        out.push_back(broadcast_binary(ctx, base, exponent, 6, 0));
        return out;
    }
};

// PRelu (src/ops/unary_elementwise.rs:624-671): x < 0 ? slope * x : x; the slope broadcasts to x's shape only
struct PRelu : Operator {
    const char *name() const override { return "PRelu"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        if (x.dtype() != DType::F32) throw OpError(OpError::UnsupportedType, "");
        const Tensor &slope = want(require(in, 1), DType::F32, "float32");
        bool ok = slope.ndim() <= x.ndim();
        for (int i = 0; ok && i < slope.ndim(); i++) {
            const int64_t sd = slope.size(slope.ndim() - 1 - i);
            ok = sd == 1 || sd == x.size(x.ndim() - 1 - i);
        }
        if (!ok) throw OpError(OpError::IncompatibleInputShapes, "Slope is not broadcastable to input shape");
        OutputList out;
        out.push_back(broadcast_binary(ctx, x, slope, 7, 0));
        return out;
    }
};

// Min / Max / Sum / Mean (src/ops/variadic_elementwise.rs:21-39): one input is a copy, otherwise a left fold of the binary operator.  Min / Max follow
// cmp_nan_less / cmp_nan_greater (reduce.rs:847-873): a NaN in either operand wins, a tie keeps the left operand.
struct Variadic : Operator {
    const char *nm;
    int f32_op, i32_op; // i32_op < 0: float32 only (Mean)
    Variadic(const char *n, int f, int i) : nm(n), f32_op(f), i32_op(i) {}
    const char *name() const override { return nm; }
    Tensor fold(Context &ctx, const InputList &in) const {
        const Tensor &first = require(in, 0);
        if (i32_op < 0) want(first, DType::F32, "float32");
        else if (first.dtype() != DType::F32 && first.dtype() != DType::I32) throw OpError(OpError::UnsupportedType, "");
        std::vector<const Tensor *> ts;
        for (const Tensor *t : in)
            if (t) ts.push_back(&want(*t, first.dtype(), first.dtype() == DType::F32 ? "float32" : "int32"));
        if (ts.size() == 1) {
            Tensor y(ctx, first.shape(), first.dtype());
            if (first.bytes()) ctx.check(rten_hip_memcpy_d2d(ctx.raw(), y.ptr(), first.ptr(), first.bytes()));
            y.set_uniform_dims(first.uniform_dims());
            return y;
        }
        Tensor acc = broadcast_binary(ctx, *ts[0], *ts[1], f32_op, i32_op);
        for (size_t k = 2; k < ts.size(); k++) acc = broadcast_binary(ctx, acc, *ts[k], f32_op, i32_op);
        return acc;
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        OutputList out;
        out.push_back(fold(ctx, in));
        return out;
    }
};
struct Min : Variadic { Min() : Variadic("Min", 4, RTEN_HIP_EW_IMIN) {} };
struct Max : Variadic { Max() : Variadic("Max", 5, RTEN_HIP_EW_IMAX) {} };
struct Sum : Variadic { Sum() : Variadic("Sum", 0, RTEN_HIP_EW_IADD) {} };
// Mean: the sum DIVIDED by n as f32 (variadic_elementwise.rs:98-102), through the Div kernel.  The divisor is a one-element device constant made on the
// first run (an upload: the warm-up run that precedes every capture makes it, a captured run finds it).
struct Mean : Variadic {
    Mean() : Variadic("Mean", 0, -1) {}
    OutputList run(Context &ctx, const InputList &in) const override {
        Tensor total = fold(ctx, in);
        size_t n = 0;
        for (const Tensor *t : in) n += t != nullptr;
        if (!divisor_ || divisor_n_ != n || divisor_ctx_ != &ctx) {
            if (rten_hip_capture_active(ctx.raw())) throw OpError(OpError::UnsupportedValue, "Mean: the divisor must be uploaded before the run is captured");
            const float d = (float)n;
            // (unpooled, as Div's reciprocals: a copy kept across runs must not come out of the pool -- taking the 4-byte buffer that an earlier step of the
            // warm-up run gave back would leave the captured run one buffer short, and an allocation inside a capture is refused)
            divisor_ = std::make_shared<Tensor>(Tensor::from_host_unpooled<float>(ctx, {}, &d));
            divisor_n_ = n;
            divisor_ctx_ = &ctx;
        }
        if (total.len()) ctx.check(rten_hip_div_f32(ctx.raw(), total.len(), (const float *)total.ptr(), (const float *)divisor_->ptr(), 1, (float *)total.ptr()));
        OutputList out;
        out.push_back(std::move(total));
        return out;
    }
  private:
    mutable std::shared_ptr<Tensor> divisor_;
    mutable size_t divisor_n_ = 0;
    mutable const Context *divisor_ctx_ = nullptr;
};

// Pad (src/ops/pad.rs).  pad_geometry: the reference's checks on a shape (pad.rs:41-124) -> the output shape; `copy` = the output equals the cropped input.
struct PadGeometry { std::vector<int64_t> out; bool copy = false; };
inline PadGeometry pad_geometry(const std::vector<int64_t> &shape, const std::vector<int64_t> &pads, int mode) {
    const size_t nd = shape.size();
    if (pads.size() != 2 * nd) throw OpError(OpError::InvalidValue, "padding length should be 2 * input dims");
    std::vector<int64_t> cropped = shape;
    for (size_t d = 0; d < nd; d++) {
        const int64_t crop = std::max<int64_t>(-pads[d], 0) + std::max<int64_t>(-pads[nd + d], 0);
        if (crop > shape[d]) throw OpError(OpError::InvalidValue, "Negative pads remove more elements than axis contains");
        cropped[d] = shape[d] - crop;
    }
    PadGeometry g;
    for (size_t d = 0; d < nd; d++) g.out.push_back(std::max<int64_t>(pads[d], 0) + cropped[d] + std::max<int64_t>(pads[nd + d], 0));
    g.copy = g.out == cropped;
    if (!g.copy && mode != RTEN_HIP_PAD_CONSTANT) {
        const size_t batch = nd > 2 ? nd - 2 : 0;
        for (size_t d = 0; d < batch; d++)
            if (g.out[d] != cropped[d]) throw OpError(OpError::UnsupportedValue, "Pad only supports non-constant padding of last 2 dims");
        for (size_t d = batch; d < nd; d++)
            if (cropped[d] == 0) throw OpError(OpError::InvalidValue, "Padded dimension for non-constant padding is empty");
    }
    return g;
}
inline int pad_mode_of(const std::string &s) { // -1: unknown
    return s == "constant" ? RTEN_HIP_PAD_CONSTANT : s == "reflect" ? RTEN_HIP_PAD_REFLECT : s == "edge" ? RTEN_HIP_PAD_EDGE : s == "wrap" ? RTEN_HIP_PAD_WRAP : -1;
}
// One rten_hip_pad_b32 launch; `fill_bits` = the constant value's word
inline Tensor pad_tensor(Context &ctx, const Tensor &x, const std::vector<int64_t> &pads, int mode, uint32_t fill_bits) {
    if (dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
    const PadGeometry g = pad_geometry(x.shape(), pads, mode);
    if (x.ndim() > 6) throw OpError(OpError::UnsupportedValue, "Pad of more than 6 dims is not supported by the device path");
    Tensor y(ctx, g.out, x.dtype());
    if (y.len()) ctx.check(rten_hip_pad_b32(ctx.raw(), mode, x.ndim(), x.shape().data(), pads.data(), fill_bits, x.ptr(), y.ptr()));
    return y;
}
// Inputs (data, pads, constant_value, axes).  pads and the constant value are read from their host values when they carry one (constants, shape
// arithmetic) and read back from the device otherwise (the graph executor refuses that case before it gets here: a read-back cannot be captured).
struct Pad : Operator {
    int mode = RTEN_HIP_PAD_CONSTANT;
    const char *name() const override { return "Pad"; }
    int max_inputs() const override { return 4; }
    static uint32_t fill_word(const Tensor &x, const Tensor *value) {
        if (!value) return 0;
        if (value->dtype() != x.dtype()) throw OpError(OpError::InputCastFailed, x.dtype() == DType::F32 ? "expected float32 tensor" : "expected int32 tensor");
        if (value->ndim() != 0) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
        uint32_t w = 0;
        if (const HostVal *h = value->host()) {
            if (h->is_float) std::memcpy(&w, &h->f.at(0), 4); else w = (uint32_t)(int32_t)h->i.at(0);
        } else {
            const std::vector<int32_t> v = value->to_host<int32_t>(); // (the raw word of either type)
            w = (uint32_t)v.at(0);
        }
        return w;
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0), &p = want(require(in, 1), DType::I32, "int32");
        if (get(in, 3)) throw OpError(OpError::UnsupportedValue, "Pad operator does not yet support `axes` input");
        if (p.ndim() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 1 dims");
        std::vector<int64_t> pads;
        if (p.host()) pads = p.host()->i;
        else for (int32_t v : p.to_host<int32_t>()) pads.push_back(v);
        OutputList out;
        out.push_back(pad_tensor(ctx, x, pads, mode, fill_word(x, get(in, 2))));
        return out;
    }
};

// Expand (src/ops/layout.rs:177-262): numpy broadcast of x against `shape` (the values of the second input, which the host must know)
inline Tensor expand_to(Context &ctx, const Tensor &x, const std::vector<int64_t> &target) {
    if (dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
    const Broadcast bc = broadcast_shapes({&x.shape(), &target});
    Tensor y(ctx, bc.shape, x.dtype());
    if (y.len()) ctx.check(rten_hip_copy_strided_b32(ctx.raw(), (int32_t)bc.shape.size(), bc.shape.data(), bc.strides[0].data(), x.ptr(), y.ptr()));
    y.set_uniform_dims(uniform_after_broadcast({&x}, bc.shape));
    return y;
}

// Slice (src/ops/slice.rs:21-118): per-axis [start, end) with a positive or negative step; clamping rules of the ONNX operator.  Returns the
// resolved (start, count, step) per axis of `shape`.
struct SliceRange { int64_t start, count, step; };
inline std::vector<SliceRange> resolve_slice(const std::vector<int64_t> &shape, const std::vector<int64_t> &starts, const std::vector<int64_t> &ends,
                                             const std::vector<int64_t> &axes, const std::vector<int64_t> &steps) {
    const int nd = (int)shape.size();
    // the reference's checks, in its order and words (slice.rs:36-60); absent axes are [0 .. r)
    if (axes.size() > (size_t)nd) throw OpError(OpError::InvalidValue, "`axes` length must be <= input rank");
    const size_t n_axes = axes.empty() ? (size_t)nd : axes.size();
    if (starts.size() != n_axes) throw OpError(OpError::InvalidValue, "`starts` length must match axis count");
    if (ends.size() != n_axes) throw OpError(OpError::InvalidValue, "`ends` length must match axis count");
    if (!steps.empty() && steps.size() != n_axes) throw OpError(OpError::InvalidValue, "`steps` length must match axis count");
    for (int64_t step : steps) if (step == 0) throw OpError(OpError::InvalidValue, "steps must be non-zero");
    std::vector<SliceRange> r((size_t)nd);
    for (int d = 0; d < nd; d++) r[(size_t)d] = {0, shape[(size_t)d], 1};
    for (size_t k = 0; k < starts.size(); k++) {
        const int ax = resolve_axis((int)(axes.empty() ? (int64_t)k : axes[k]), nd);
        const int64_t dim = shape[(size_t)ax], step = steps.empty() ? 1 : steps[k];
        int64_t st = starts[k], en = ends[k];
        if (st < 0) st += dim;
        if (en < 0) en += dim;
        if (step > 0) {
            st = std::min(std::max<int64_t>(st, 0), dim);
            en = std::min(std::max<int64_t>(en, 0), dim);
            r[(size_t)ax] = {st, en > st ? (en - st + step - 1) / step : 0, step};
        } else {
            st = std::min(std::max<int64_t>(st, -1), dim - 1);
            en = std::min(std::max<int64_t>(en, -1), dim - 1);
            r[(size_t)ax] = {st, st > en ? (st - en + (-step) - 1) / (-step) : 0, step};
        }
    }
    return r;
}
inline Tensor slice_tensor(Context &ctx, const Tensor &x, const std::vector<SliceRange> &r) {
    if (dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
    const int nd = x.ndim();
    if (nd > 6) throw OpError(OpError::UnsupportedValue, "Slice: more than 6 dims on the device path");
    std::vector<int64_t> oshape((size_t)nd), st((size_t)nd);
    int64_t acc = 1, base = 0;
    bool forward = true;
    for (int d = nd - 1; d >= 0; d--) {
        oshape[(size_t)d] = r[(size_t)d].count;
        st[(size_t)d] = acc * r[(size_t)d].step;
        base += acc * r[(size_t)d].start;
        if (r[(size_t)d].step < 0) forward = false;
        acc *= x.size(d);
    }
    Tensor y(ctx, oshape, x.dtype());
    if (!y.len()) return y;
    if (forward) {
        ctx.check(rten_hip_copy_strided_b32(ctx.raw(), nd, oshape.data(), st.data(), (const char *)x.ptr() + base * 4, y.ptr()));
    } else { // negative steps: the strided-copy entry point takes non-negative strides; the generic kernel takes signed ones (Cast int32 -> int32 moves raw words)
        const int32_t dt = RTEN_HIP_DT_I32;
        ctx.check(rten_hip_elementwise_nd(ctx.raw(), RTEN_HIP_EW_IADD, nd, oshape.data(), (const char *)x.ptr() + base * 4, dt, st.data(), ctx.zero_i32(), dt,
                                          std::vector<int64_t>((size_t)nd, 0).data(), nullptr, nullptr, y.ptr(), dt));
    }
    return y;
}

// Concat (src/ops/concat.rs:21-108) of 4-byte tensors along `axis`
inline Tensor concat_tensors(Context &ctx, const InputList &in, int axis) {
    const Tensor &first = require(in, 0);
    const int nd = first.ndim();
    const int ax = resolve_axis(axis, nd);
    std::vector<int64_t> oshape = first.shape();
    oshape[(size_t)ax] = 0;
    for (size_t k = 0; k < in.size(); k++) {
        const Tensor &t = require(in, k);
        if (t.dtype() != first.dtype() || dtype_size(t.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
        if (t.ndim() != nd) throw OpError(OpError::IncompatibleInputShapes, "Tensors must have the same number of dimensions");
        for (int d = 0; d < nd; d++) if (d != ax && t.size(d) != first.size(d)) throw OpError(OpError::IncompatibleInputShapes, "Dimensions must be the same except for concat axis");
        oshape[(size_t)ax] += t.size(ax);
    }
    Tensor y(ctx, oshape, first.dtype());
    const int64_t outer = detail::prod(oshape, 0, (size_t)ax), inner = detail::prod(oshape, (size_t)ax + 1, oshape.size());
    const int64_t dst_pitch = oshape[(size_t)ax] * inner;
    int64_t off = 0;
    for (size_t k = 0; k < in.size(); k++) {
        const int64_t row = in[k]->size(ax) * inner;
        if (row && outer) ctx.check(rten_hip_copy_rows_b32(ctx.raw(), outer, row, in[k]->ptr(), row, (char *)y.ptr() + off * 4, dst_pitch));
        off += row;
    }
    return y;
}

// ------------------------------------------------------------------------------------------------ Resize / Upsample / Split
// Resize's target (src/ops/resize.rs:20-27): a scale (f32) or an output size (i32) per input dim.
struct ResizeTarget {
    bool scales = true;
    std::vector<float> s;
    std::vector<int64_t> n;
};
// calc_output_size (resize.rs:273-308): size = floor(in * scale) in f32 (`as i32` saturates, NaN -> 0) and inv_scale = 1 / scale, or size and in / size
inline void resize_geometry(const std::vector<int64_t> &in, const ResizeTarget &t, std::vector<int64_t> &sizes, std::vector<float> &inv) {
    if ((t.scales ? t.s.size() : t.n.size()) != in.size()) throw OpError(OpError::IncompatibleInputShapes, "scales/sizes length should equal input rank");
    sizes.assign(in.size(), 0);
    inv.assign(in.size(), 0.f);
    for (size_t i = 0; i < in.size(); i++) {
        if (t.scales) {
            const float f = std::floor((float)in[i] * t.s[i]);
            sizes[i] = f != f ? 0 : f >= 2147483648.f ? INT32_MAX : f < -2147483648.f ? INT32_MIN : (int64_t)f;
            inv[i] = 1.f / t.s[i];
        } else {
            const int32_t o = (int32_t)t.n[i];
            sizes[i] = o;
            inv[i] = (float)in[i] / (float)o;
        }
    }
    for (int64_t v : sizes) if (v < 0) throw OpError(OpError::InvalidValue, "scales/sizes must be positive");
}

// Resize (resize.rs:470-606): f32 only; the input is viewed as [planes, H, W] (resize_impl, resize.rs:334-408) and resampled by rten_hip_resize_f32.
struct Resize : Operator {
    int32_t mode = RTEN_HIP_RESIZE_MODE_NEAREST, coord_mode = RTEN_HIP_RESIZE_COORD_HALF_PIXEL, nearest_mode = RTEN_HIP_RESIZE_NEAREST_ROUND_PREFER_FLOOR;
    const char *name() const override { return "Resize"; }
    int max_inputs() const override { return 4; }
    // inputs X, roi (read by tf_crop_and_resize only, which the loader refuses), scales, sizes
    OutputList run(Context &ctx, const InputList &in) const override {
        OutputList out;
        out.push_back(resize(ctx, require(in, 0), target(get(in, 2), get(in, 3))));
        return out;
    }
    // target_from_scale_size_inputs (resize.rs:312-325, 496-507): an absent or empty tensor is missing.  Values come from the tensor's host mirror
    // when it has one (constants, shape arithmetic), else they are read back.
    static ResizeTarget target(const Tensor *scales, const Tensor *sizes) {
        const bool has_s = scales && scales->len(), has_n = sizes && sizes->len();
        if (has_s && scales->ndim() != 1) throw OpError(OpError::InvalidValue, "scales must have 1 dims");
        if (has_n && sizes->ndim() != 1) throw OpError(OpError::InvalidValue, "sizes must have 1 dims");
        if (has_s) return scales_target(*scales);
        if (!has_n) throw OpError(OpError::MissingInputs, "");
        want(*sizes, DType::I32, "int32");
        ResizeTarget t;
        t.scales = false;
        if (sizes->host()) t.n = sizes->host()->i;
        else for (int32_t v : sizes->to_host<int32_t>()) t.n.push_back(v);
        return t;
    }
    static ResizeTarget scales_target(const Tensor &scales) {
        if (scales.ndim() != 1) throw OpError(OpError::InvalidValue, "scales must have 1 dims");
        want(scales, DType::F32, "float32");
        ResizeTarget t;
        t.s = scales.host() ? scales.host()->f : scales.to_host<float>();
        return t;
    }
    Tensor resize(Context &ctx, const Tensor &x_in, const ResizeTarget &t) const {
        const Tensor &x = want(x_in, DType::F32, "float32");
        std::vector<int64_t> os;
        std::vector<float> inv;
        resize_geometry(x.shape(), t, os, inv);
        const std::vector<int64_t> &is = x.shape();
        if (os == is) { // nothing resized: a copy, whatever the scales were (resize.rs:352)
            Tensor y(ctx, os, DType::F32);
            if (y.bytes()) ctx.check(rten_hip_memcpy_d2d(ctx.raw(), y.ptr(), x.ptr(), y.bytes()));
            return y;
        }
        int64_t planes = 1, ih = 1, iw = 1, oh = 1, ow = 1;
        float sy = 1.f, sx = 1.f; // an axis the input is expanded along is not resized: scale 1
        const size_t nd = is.size();
        if (nd == 4 && is[0] == os[0] && is[1] == os[1]) { planes = is[0] * is[1]; ih = is[2]; iw = is[3]; oh = os[2]; ow = os[3]; sy = inv[2]; sx = inv[3]; }
        else if (nd == 3 && is[0] == os[0] && is[1] == os[1]) { planes = is[0] * is[1]; iw = is[2]; ow = os[2]; sx = inv[2]; } // NCW (tried first)
        else if (nd == 3 && is[0] == os[0]) { planes = is[0]; ih = is[1]; iw = is[2]; oh = os[1]; ow = os[2]; sy = inv[1]; sx = inv[2]; } // NHW
        else if (nd == 2) { ih = is[0]; iw = is[1]; oh = os[0]; ow = os[1]; sy = inv[0]; sx = inv[1]; }
        else if (nd == 1) { iw = is[0]; ow = os[0]; sx = inv[0]; }
        else throw OpError(OpError::UnsupportedValue, "Only 1D to 4D inputs are supported with up to two resized dimensions");
        Tensor y(ctx, os, DType::F32);
        if (y.len())
            ctx.check(rten_hip_resize_f32(ctx.raw(), mode, coord_mode, nearest_mode, planes, ih, iw, oh, ow, sy, sx, (const float *)x.ptr(), (float *)y.ptr()));
        return y;
    }
};

// Upsample (resize.rs:610-652): the deprecated form of Resize -- scales required (input 1), asymmetric coordinates, floor.
struct Upsample : Resize {
    Upsample() { coord_mode = RTEN_HIP_RESIZE_COORD_ASYMMETRIC; nearest_mode = RTEN_HIP_RESIZE_NEAREST_FLOOR; }
    const char *name() const override { return "Upsample"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        OutputList out;
        out.push_back(resize(ctx, require(in, 0), scales_target(require(in, 1))));
        return out;
    }
};

// GridSample (src/ops/grid_sample.rs:17-145): bilinear sampling with zero padding of X [N, C, H, W] at grid [N, H_out, W_out, 2]; one
// rten_hip_grid_sample_f32 launch (rten_amd/csrc/sample.hip).  The loaders refuse every other mode / padding_mode (onnx_registry.rs:1203-1212).
struct GridSample : Operator {
    bool align_corners = false;
    const char *name() const override { return "GridSample"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        if (x.ndim() != 4) throw OpError(OpError::InvalidValue, "input must have 4 dims (NCHW)");
        const Tensor &grid = want(require(in, 1), DType::F32, "float32");
        if (grid.ndim() != 4) throw OpError(OpError::InvalidValue, "grid must have 4 dims");
        if (grid.size(0) != x.size(0)) throw OpError(OpError::IncompatibleInputShapes, "Batch size of input and grid must match");
        if (grid.size(3) != 2) throw OpError(OpError::UnsupportedValue, "Unsupported grid coordinate size");
        Tensor y(ctx, {x.size(0), x.size(1), grid.size(1), grid.size(2)}, DType::F32);
        if (y.len())
            ctx.check(rten_hip_grid_sample_f32(ctx.raw(), align_corners ? 1 : 0, x.size(0), x.size(1), x.size(2), x.size(3), grid.size(1), grid.size(2), (const float *)x.ptr(),
                                               (const float *)grid.ptr(), (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// DepthToSpace (src/ops/layout.rs:22-103): the permutation of the ONNX specification as ONE rten_hip_transpose_b32 launch on the 6-D view the
// reference builds -- DCR [n, b, b, c', h, w] by (0, 3, 4, 1, 5, 2), CRD [n, c', b, b, h, w] by (0, 1, 4, 2, 5, 3) -- read as [n, c', h * b, w * b].
// float32 only, as the reference's run().
enum class DepthToSpaceMode { DepthColumnRow, ColumnRowDepth };
struct DepthToSpace : Operator {
    int64_t block_size = 0; // the attribute is required (onnx_registry.rs:1106)
    DepthToSpaceMode mode = DepthToSpaceMode::DepthColumnRow;
    const char *name() const override { return "DepthToSpace"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        if (block_size <= 0) throw OpError(OpError::InvalidValue, "`block_size` must be > 0");
        if (x.ndim() != 4) throw OpError(OpError::InvalidValue, "input must have 4 dims (NCHW)");
        const int64_t n = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3), b = block_size;
        if (b > 0x7fffffff || c % (b * b) != 0) throw OpError(OpError::InvalidValue, "input channels must be a multiple of `block_size` squared");
        const int64_t nc = c / (b * b);
        const bool dcr = mode == DepthToSpaceMode::DepthColumnRow;
        const std::vector<int64_t> view = dcr ? std::vector<int64_t>{n, b, b, nc, h, w} : std::vector<int64_t>{n, nc, b, b, h, w};
        const int32_t dcr_perm[6] = {0, 3, 4, 1, 5, 2}, crd_perm[6] = {0, 1, 4, 2, 5, 3};
        Tensor y(ctx, {n, nc, h * b, w * b}, DType::F32);
        if (y.len()) ctx.check(rten_hip_transpose_b32(ctx.raw(), 6, view.data(), dcr ? dcr_perm : crd_perm, x.ptr(), y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// ---- CumSum, GatherElements, Trilu, Tile (rten_amd/csrc/scan.hip): float32 / int32 data (booleans are int32), rank <= 6, one launch each, nothing read back
inline void want_b32_numeric(const Tensor &x) {
    if (x.dtype() != DType::F32 && x.dtype() != DType::I32) throw OpError(OpError::UnsupportedType, "");
}
// a one-element int32 operand (the reference's `require_as::<i32>`: any rank, one element): from its host value, else read back
inline int64_t scalar_i32(const Tensor &t) {
    want(t, DType::I32, "int32");
    if (t.len() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
    if (t.host()) return t.host()->i.at(0);
    return t.to_host<int32_t>().at(0);
}
// cum_sum (reduce.rs:217-257): a rank-0 operand is resolve_axis's "Axis is invalid"; an empty tensor launches nothing
inline Tensor cumsum_tensor(Context &ctx, const Tensor &x, int64_t axis, bool exclusive, bool reverse) {
    want_b32_numeric(x);
    if (axis < INT32_MIN || axis > INT32_MAX) throw OpError(OpError::InvalidValue, "Axis is invalid");
    const int ax = resolve_axis((int)axis, x.ndim());
    const int64_t outer = detail::prod(x.shape(), 0, (size_t)ax), inner = detail::prod(x.shape(), (size_t)ax + 1, x.shape().size());
    Tensor y(ctx, x.shape(), x.dtype());
    if (y.len())
        ctx.check(rten_hip_cumsum_b32(ctx.raw(), x.dtype() == DType::F32 ? RTEN_HIP_DTYPE_F32 : RTEN_HIP_DTYPE_I32, exclusive ? 1 : 0, reverse ? 1 : 0, outer, x.size(ax), inner,
                                      x.ptr(), y.ptr()));
    return y;
}
// gather_elements' shape checks (gather.rs:202-217), shared by the host and the device path: -> the resolved axis
inline int check_gather_elements(const std::vector<int64_t> &x_shape, const std::vector<int64_t> &idx_shape, int axis) {
    if (x_shape.size() != idx_shape.size()) throw OpError(OpError::IncompatibleInputShapes, "Input and indices must have same rank");
    const int ax = resolve_axis(axis, (int)x_shape.size());
    for (size_t d = 0; d < x_shape.size(); d++)
        if ((int)d != ax && idx_shape[d] > x_shape[d]) throw OpError(OpError::IncompatibleInputShapes, "`indices` size must be <= input size in non-axis dimensions");
    return ax;
}
// Out-of-range indices: host-valued indices are checked here with the reference's message; device indices are clamped by the kernel (the deviation
// rten_hip_gather_axis_b32 documents for Gather: nothing is read back).
inline Tensor gather_elements_tensor(Context &ctx, const Tensor &x, const Tensor &ids, int axis) {
    want(ids, DType::I32, "int32");
    if (dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
    const int ax = check_gather_elements(x.shape(), ids.shape(), axis);
    if (x.ndim() > 6) throw OpError(OpError::UnsupportedValue, "GatherElements supports at most 6 dims");
    const int64_t alen = x.size(ax);
    if (ids.len() && alen == 0) throw OpError(OpError::InvalidValue, "Entry in `indices` is out of range");
    if (const HostVal *h = ids.host())
        for (int64_t id : h->i) if (id < -alen || id >= alen) throw OpError(OpError::InvalidValue, "Entry in `indices` is out of range");
    Tensor y(ctx, ids.shape(), x.dtype());
    if (y.len()) ctx.check(rten_hip_gather_elements_b32(ctx.raw(), x.ndim(), x.shape().data(), ids.shape().data(), ax, x.ptr(), (const int32_t *)ids.ptr(), y.ptr()));
    return y;
}
inline Tensor trilu_tensor(Context &ctx, const Tensor &x, int64_t k, bool upper) {
    want_b32_numeric(x);
    if (x.ndim() < 2) throw OpError(OpError::InvalidValue, "Input must have >= 2 dims");
    const int nd = x.ndim();
    Tensor y(ctx, x.shape(), x.dtype());
    if (y.len()) ctx.check(rten_hip_trilu_b32(ctx.raw(), upper ? 1 : 0, k, detail::prod(x.shape(), 0, (size_t)nd - 2), x.size(nd - 2), x.size(nd - 1), x.ptr(), y.ptr()));
    return y;
}
// tile's check (concat.rs:244-246) and output shape
inline std::vector<int64_t> tiled_shape(const std::vector<int64_t> &shape, const std::vector<int64_t> &repeats) {
    if (repeats.size() != shape.size()) throw OpError(OpError::InvalidValue, "invalid repeats");
    for (int64_t r : repeats) if (r < 0) throw OpError(OpError::InvalidValue, "invalid repeats");
    std::vector<int64_t> out(shape);
    for (size_t d = 0; d < out.size(); d++) out[d] *= repeats[d];
    return out;
}
inline Tensor tile_tensor(Context &ctx, const Tensor &x, const std::vector<int64_t> &repeats) {
    want_b32_numeric(x);
    const std::vector<int64_t> oshape = tiled_shape(x.shape(), repeats);
    if (x.ndim() > 6) throw OpError(OpError::UnsupportedValue, "Tile supports at most 6 dims");
    Tensor y(ctx, oshape, x.dtype());
    if (y.len()) ctx.check(rten_hip_tile_b32(ctx.raw(), x.ndim(), x.shape().data(), repeats.data(), x.ptr(), y.ptr()));
    return y;
}

// CumSum (src/ops/reduce.rs:259-297): inputs (data, axis); the axis is a one-element int32 operand, read from its host value when it carries one (a
// constant, shape arithmetic) and read back otherwise (the graph executor refuses that case before it gets here: a read-back cannot be captured).
struct CumSum : Operator {
    bool exclusive = false, reverse = false;
    const char *name() const override { return "CumSum"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        const int64_t axis = scalar_i32(require(in, 1));
        OutputList out;
        out.push_back(cumsum_tensor(ctx, x, axis, exclusive, reverse));
        return out;
    }
};
// GatherElements (src/ops/gather.rs:196-319): y[i0, ..] = x[i0, .., indices[i0, ..], ..] along `axis`, on the input trimmed to the indices' extent
struct GatherElements : Operator {
    int axis = 0;
    const char *name() const override { return "GatherElements"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0), &ids = require(in, 1);
        OutputList out;
        out.push_back(gather_elements_tensor(ctx, x, ids, axis));
        return out;
    }
};
// Trilu (src/ops/trilu.rs:66-97): inputs (data, k); k is optional, default 0, read like CumSum's axis
struct Trilu : Operator {
    bool upper = true;
    const char *name() const override { return "Trilu"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        const int64_t k = get(in, 1) ? scalar_i32(*get(in, 1)) : 0;
        OutputList out;
        out.push_back(trilu_tensor(ctx, x, k, upper));
        return out;
    }
};
// Tile (src/ops/concat.rs:274-295): inputs (data, repeats); repeats is a 1-D int32 operand read like Pad's pads
struct Tile : Operator {
    const char *name() const override { return "Tile"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0), &r = want(require(in, 1), DType::I32, "int32");
        if (r.ndim() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 1 dims");
        std::vector<int64_t> repeats;
        if (r.host()) repeats = r.host()->i;
        else for (int32_t v : r.to_host<int32_t>()) repeats.push_back(v);
        OutputList out;
        out.push_back(tile_tensor(ctx, x, repeats));
        return out;
    }
};

// ---- NonMaxSuppression (src/ops/non_max_suppression.rs:40-233; rten_amd/csrc/nms.hip): inputs boxes [N, B, 4], scores [N, C, B] and three optional
// one-element operands, max_output_boxes_per_class (int32; ABSENT = no limit, the reference's default), iou_threshold and score_threshold (float32, 0).
// The three are HOST values -- constants or shape arithmetic, read the way Slice reads its starts -- and a device-valued one is refused: the reference's
// get_as (operator.rs:790-806; one element of any rank, else "expected tensor with 0 dims").  The result is int32 [count, 3], rows [n, class, b]: the
// first operator here whose output SHAPE depends on device values, so the call synchronises once (the count) and cannot be captured into a graph.
inline void check_nms_shapes(const std::vector<int64_t> &boxes, const std::vector<int64_t> &scores) {
    if (boxes.size() != 3 || scores.size() != 3) throw OpError(OpError::InputCastFailed, "expected tensor with 3 dims");
    if (boxes[2] != 4) throw OpError(OpError::InvalidValue, "`boxes` last dimension should have size 4");
    if (boxes[0] != scores[0] || boxes[1] != scores[2]) throw OpError(OpError::IncompatibleInputShapes, "`boxes` and `scores` have incompatible shapes");
}
// one optional scalar operand: false when absent
inline const HostVal *nms_scalar(const InputList &in, size_t i, bool is_float, const char *what) {
    const Tensor *t = get(in, i);
    if (!t) return nullptr;
    want(*t, is_float ? DType::F32 : DType::I32, is_float ? "float32" : "int32");
    if (t->len() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
    if (!t->host() || t->host()->is_float != is_float)
        throw OpError(OpError::UnsupportedValue, std::string("NonMaxSuppression: ") + what + " must be a constant or computable from the input shapes (it depends on device data)");
    return t->host();
}
inline Tensor nms_tensor(Context &ctx, const Tensor &boxes, const Tensor &scores, int center_point_box, bool has_max, int64_t max_per_class, float iou_threshold, float score_threshold) {
    want(boxes, DType::F32, "float32");
    want(scores, DType::F32, "float32");
    check_nms_shapes(boxes.shape(), scores.shape());
    if (center_point_box != 0 && center_point_box != 1) throw OpError(OpError::InvalidValue, "center_point_box must be 0 or 1");
    const int64_t n = boxes.size(0), b = boxes.size(1), c = scores.size(1);
    if (c == 0 || n * b == 0) return Tensor(ctx, {0, 3}, DType::I32);
    Tensor rows(ctx, {n * b, 3}, DType::I32);
    int64_t count = 0;
    const int64_t cap = std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, max_per_class)); // the loader's saturating int64 -> int32
    ctx.check(rten_hip_non_max_suppression_f32(ctx.raw(), center_point_box, n, c, b, (const float *)boxes.ptr(), (const float *)scores.ptr(), has_max ? 1 : 0, (int32_t)cap,
                                               iou_threshold, score_threshold, (int32_t *)rows.ptr(), &count));
    rows.reshape({count, 3}); // (the buffer keeps its capacity of n * b rows)
    return rows;
}
struct NonMaxSuppression : Operator {
    int center_point_box = 0;
    const char *name() const override { return "NonMaxSuppression"; }
    int max_inputs() const override { return 5; }
    OutputList run(Context &ctx, const InputList &in) const override {
        if (in.size() > 5) throw OpError(OpError::InvalidValue, "NonMaxSuppression takes at most 5 inputs");
        const Tensor &boxes = require(in, 0), &scores = require(in, 1);
        const HostVal *cap = nms_scalar(in, 2, false, "max_output_boxes_per_class"), *iou = nms_scalar(in, 3, true, "iou_threshold"), *score = nms_scalar(in, 4, true, "score_threshold");
        OutputList out;
        out.push_back(nms_tensor(ctx, boxes, scores, center_point_box, cap != nullptr, cap ? cap->i.at(0) : 0, iou ? iou->f.at(0) : 0.f, score ? score->f.at(0) : 0.f));
        return out;
    }
};

// ---- DFT and STFT (src/ops/fft.rs:22-373; rten_amd/csrc/fft.hip): float32, one LDS-resident Stockham FFT behind both.  dft_length, axis, frame_step and
// frame_length are HOST values -- constants or shape arithmetic -- and a device-valued one is refused.  The contract is an error bound against the exact
// transform (include/rten_hip.h), not bit-identity with the reference's FFT library.  Lengths above RTEN_HIP_FFT_MAX are UnsupportedValue.
inline bool fft_host_int(const InputList &in, size_t i, const char *op, const char *what, int64_t *value) {
    const Tensor *t = get(in, i);
    if (!t) return false;
    want(*t, DType::I32, "int32");
    if (t->len() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
    if (!t->host() || t->host()->is_float)
        throw OpError(OpError::UnsupportedValue, std::string(op) + ": " + what + " must be a constant or computable from the input shapes (it depends on device data)");
    *value = t->host()->i.at(0);
    return true;
}
inline void fft_limit(const char *op, const char *what, int64_t n) {
    if (n > RTEN_HIP_FFT_MAX)
        throw OpError(OpError::UnsupportedValue, std::string(op) + " " + what + " of length " + std::to_string(n) + " exceeds the limit of " + std::to_string(RTEN_HIP_FFT_MAX) + " points (RTEN_HIP_FFT_MAX)");
}
// the reference's checks, in its order (fft.rs:208-258); returns the resolved axis and n_fft
inline void check_dft(const std::vector<int64_t> &shape, bool has_length, int64_t dft_length, int64_t axis, bool inverse, bool onesided, int *ax_out, int64_t *n_fft_out) {
    const int nd = (int)shape.size();
    if (nd < 2) throw OpError(OpError::InvalidValue, "DFT input must have at least 2 dims");
    const int64_t comp = shape[(size_t)nd - 1];
    if (comp != 1 && comp != 2) throw OpError(OpError::InvalidValue, "Last dimension of DFT input must have size 1 or 2");
    const bool irfft = inverse && onesided;
    if (irfft && comp != 2) throw OpError(OpError::InvalidValue, "Inverse one-sided DFT (IRFFT) requires complex input");
    if (onesided && !inverse && comp == 2) throw OpError(OpError::InvalidValue, "DFT cannot be one-sided if input is complex");
    if (axis < INT32_MIN || axis > INT32_MAX) throw OpError(OpError::InvalidValue, "Axis is invalid");
    const int ax = resolve_axis((int)axis, nd);
    if (ax == nd - 1) throw OpError(OpError::InvalidValue, "DFT axis cannot be the complex dimension");
    const int64_t n_in = shape[(size_t)ax];
    int64_t n_fft;
    if (has_length) {
        if (dft_length < 1) throw OpError(OpError::InvalidValue, "dft_length must be >= 1");
        n_fft = dft_length;
    } else {
        n_fft = irfft ? 2 * std::max<int64_t>(n_in - 1, 0) : n_in;
    }
    *ax_out = ax;
    *n_fft_out = n_fft;
}
inline Tensor dft_tensor(Context &ctx, const Tensor &x, bool has_length, int64_t dft_length, int64_t axis, bool inverse, bool onesided) {
    want(x, DType::F32, "float32");
    int ax = 0;
    int64_t n_fft = 0;
    check_dft(x.shape(), has_length, dft_length, axis, inverse, onesided, &ax, &n_fft);
    fft_limit("DFT", "transform", n_fft);
    const int nd = x.ndim();
    const bool irfft = inverse && onesided;
    const int64_t n_in = x.size(ax), comp = x.size(nd - 1), out_len = (onesided && !inverse) ? n_fft / 2 + 1 : n_fft, out_comp = irfft ? 1 : 2;
    std::vector<int32_t> fwd, back((size_t)nd);
    for (int d = 0; d < nd; d++) if (d != ax && d != nd - 1) fwd.push_back(d);
    fwd.push_back(ax);
    fwd.push_back(nd - 1);
    for (int d = 0; d < nd; d++) back[(size_t)fwd[(size_t)d]] = d;
    std::vector<int64_t> tshape, oshape_t;
    for (int d = 0; d < nd; d++) tshape.push_back(x.size(fwd[(size_t)d]));
    oshape_t = tshape;
    oshape_t[(size_t)nd - 2] = out_len;
    oshape_t[(size_t)nd - 1] = out_comp;
    const int64_t lanes = detail::prod(tshape, 0, (size_t)nd - 2);
    if (ax == nd - 2) {
        Tensor y(ctx, oshape_t, DType::F32);
        if (y.len()) ctx.check(rten_hip_dft_f32(ctx.raw(), lanes, n_in, n_fft, (int32_t)comp, inverse ? 1 : 0, onesided ? 1 : 0, (const float *)x.ptr(), (float *)y.ptr()));
        return y;
    }
    // the reference permutes the axis next to the complex dimension, transforms contiguous lanes, and permutes back (fft.rs:275-283, 360-372)
    if (nd > 6) throw OpError(OpError::UnsupportedValue, "DFT along an axis other than ndim - 2 of more than 6 dims is not supported by the device path");
    std::vector<int64_t> oshape((size_t)nd);
    for (int d = 0; d < nd; d++) oshape[(size_t)d] = oshape_t[(size_t)back[(size_t)d]];
    Tensor y(ctx, oshape, DType::F32);
    if (y.len()) {
        Tensor t(ctx, tshape, DType::F32), u(ctx, oshape_t, DType::F32);
        if (x.len()) ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, x.shape().data(), fwd.data(), x.ptr(), t.ptr()));
        ctx.check(rten_hip_dft_f32(ctx.raw(), lanes, n_in, n_fft, (int32_t)comp, inverse ? 1 : 0, onesided ? 1 : 0, (const float *)t.ptr(), (float *)u.ptr()));
        ctx.check(rten_hip_transpose_b32(ctx.raw(), nd, oshape_t.data(), back.data(), u.ptr(), y.ptr()));
    }
    return y;
}
struct DFT : Operator {
    bool inverse = false, onesided = false;
    const char *name() const override { return "DFT"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        int64_t dft_length = 0, axis = -2;
        const bool has_length = fft_host_int(in, 1, "DFT", "dft_length", &dft_length);
        fft_host_int(in, 2, "DFT", "axis", &axis);
        OutputList out;
        out.push_back(dft_tensor(ctx, x, has_length, dft_length, axis, inverse, onesided));
        return out;
    }
};
// the reference's checks, in its order (fft.rs:30-93); returns batch, signal_len, components and n_fft.  window_len < 0: no window.
inline void check_stft(const std::vector<int64_t> &signal, int64_t frame_step, int64_t window_len, bool has_frame_length, int64_t frame_length, bool onesided, int64_t *batch,
                       int64_t *signal_len, int64_t *comp, int64_t *n_fft) {
    if (signal.size() != 2 && signal.size() != 3) throw OpError(OpError::InvalidValue, "signal must have 2 or 3 dims");
    *batch = signal[0];
    *signal_len = signal[1];
    *comp = signal.size() == 3 ? signal[2] : 1;
    if (has_frame_length && (frame_length < 1 || frame_length > *signal_len)) throw OpError(OpError::InvalidValue, "frame_length must be in range [1, signal_length]");
    if (frame_step <= 0) throw OpError(OpError::InvalidValue, "frame_step must be > 0");
    if (has_frame_length && window_len >= 0 && frame_length != window_len) throw OpError(OpError::InvalidValue, "window length must equal frame_length");
    if (!has_frame_length && window_len < 0) throw OpError(OpError::InvalidValue, "Either frame_length or window must be set");
    *n_fft = has_frame_length ? frame_length : window_len;
    if (*comp != 1 && *comp != 2) throw OpError(OpError::InvalidValue, "Last dimension of signal must have size 1 or 2");
    if (*comp == 2 && onesided) throw OpError(OpError::InvalidValue, "FFT cannot be one-sided if input is complex");
    // (a window that is empty or longer than the signal: the reference's frame count is meaningless there)
    if (*n_fft < 1 || *n_fft > *signal_len) throw OpError(OpError::InvalidValue, "frame_length must be in range [1, signal_length]");
}
inline Tensor stft_tensor(Context &ctx, const Tensor &signal, int64_t frame_step, const Tensor *window, bool has_frame_length, int64_t frame_length, bool onesided) {
    want(signal, DType::F32, "float32");
    if (window) {
        want(*window, DType::F32, "float32");
        if (window->ndim() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 1 dims");
    }
    int64_t batch = 0, signal_len = 0, comp = 0, n_fft = 0;
    check_stft(signal.shape(), frame_step, window ? window->size(0) : -1, has_frame_length, frame_length, onesided, &batch, &signal_len, &comp, &n_fft);
    fft_limit("STFT", "frame", n_fft);
    const int64_t n_frames = (signal_len - n_fft) / frame_step + 1, bins = onesided ? n_fft / 2 + 1 : n_fft;
    Tensor y(ctx, {batch, n_frames, bins, 2}, DType::F32);
    if (y.len())
        ctx.check(rten_hip_stft_f32(ctx.raw(), batch, signal_len, (int32_t)comp, frame_step, n_fft, onesided ? 1 : 0, window ? (const float *)window->ptr() : nullptr,
                                    (const float *)signal.ptr(), (float *)y.ptr()));
    return y;
}
struct STFT : Operator {
    bool onesided = true;
    const char *name() const override { return "STFT"; }
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &signal = require(in, 0);
        int64_t frame_step = 0, frame_length = 0;
        if (!fft_host_int(in, 1, "STFT", "frame_step", &frame_step)) throw OpError(OpError::MissingInputs, "");
        const bool has_frame_length = fft_host_int(in, 3, "STFT", "frame_length", &frame_length);
        OutputList out;
        out.push_back(stft_tensor(ctx, signal, frame_step, get(in, 2), has_frame_length, frame_length, onesided));
        return out;
    }
};

// Split (src/ops/split.rs:34-136) of 4-byte tensors, one strided copy per piece: the sizes of input 1 (the opset < 13 `split` attribute arrives
// there too), else `num_outputs` (opset 18), else the node's output count, as equal chunks of ceil(dim / n) -- the last piece is smaller, and there
// may be fewer than n pieces (5 split 4 ways gives 3).
struct Split : Operator {
    int axis = 0;
    int64_t num_outputs = -1; // < 0: the attribute is absent
    int64_t node_outputs = 1; // outputs of the graph node (ctx.outputs().len() in the reference)
    const char *name() const override { return "Split"; }
    int max_inputs() const override { return 2; }
    // (start, length) along the axis of every piece
    std::vector<std::pair<int64_t, int64_t>> pieces(int64_t dim, const std::vector<int64_t> *sizes) const {
        std::vector<std::pair<int64_t, int64_t>> p;
        if (sizes) {
            for (int64_t s : *sizes) if (s < 0) throw OpError(OpError::InvalidValue, "Split sizes must be >= 0");
            int64_t start = 0;
            for (int64_t s : *sizes) { p.push_back({start, s}); start += s; }
            if (start != dim) throw OpError(OpError::InvalidValue, "Split sizes do not sum to dimension size");
            return p;
        }
        const int64_t n = num_outputs >= 0 ? num_outputs : node_outputs;
        if (n == 0) throw OpError(OpError::InvalidValue, "num_outputs must be > 0");
        if (n > dim) throw OpError(OpError::InvalidValue, "num_outputs exceeds dim size");
        const int64_t chunk = (dim + n - 1) / n;
        for (int64_t s = 0; s < dim; s += chunk) p.push_back({s, std::min(chunk, dim - s)});
        return p;
    }
    static std::vector<SliceRange> piece_ranges(const Tensor &x, int a, const std::pair<int64_t, int64_t> &pc) {
        std::vector<SliceRange> r;
        for (int d = 0; d < x.ndim(); d++) r.push_back({0, x.size(d), 1});
        r[(size_t)a] = {pc.first, pc.second, 1};
        return r;
    }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0);
        const int a = resolve_axis(axis, x.ndim());
        const Tensor *s = get(in, 1);
        std::vector<int64_t> sizes;
        if (s) {
            want(*s, DType::I32, "int32");
            if (s->host()) sizes = s->host()->i;
            else for (int32_t v : s->to_host<int32_t>()) sizes.push_back(v);
        }
        OutputList out;
        for (auto &pc : pieces(x.size(a), s ? &sizes : nullptr)) out.push_back(slice_tensor(ctx, x, piece_ranges(x, a, pc)));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ Einsum / ReduceSum
// src/ops/einsum.rs:21-692, rten-shape-inference/src/einsum_parser.rs:68-275, src/ops/reduce.rs:414-520,1101-1165.
// The reference walks a path of two-term steps over permuted TensorViews and copies where a kernel wants contiguous data.
// Here a view is (device pointer, shape, element strides) and the kernels read THROUGH the strides: permutes, inserted axes,
// diagonals and 1 -> n expansion are stride arithmetic; ReduceSum runs in place on the strided view; a product is ONE
// rten_hip_gemm_f32 launch (M / K / N are strides, batch labels become the descriptor's two batch levels once neighbouring
// axes with compatible strides are merged); the final permutation into the output order goes into the GEMM's C strides when it
// keeps N innermost and is a copy otherwise.  The order of the
// arithmetic is the reference's (same path, same M / N / batch labels, lone labels summed first, [A, M, K] x [K, N] folded
// into one GEMM), so results are bit-identical except for a GEMM with one row (ISA-dependent gemv path).
namespace einsum_detail {
using Shape = std::vector<int64_t>;
constexpr char INS_M = '<', INS_N = '>', MERGED_K = '*'; // einsum.rs:366-380
constexpr int MAX_DIMS = 10;                             // einsum_parser.rs:241-245

inline bool has(const std::string &s, char c) { return s.find(c) != std::string::npos; }
inline std::string dedup(const std::string &s) {
    std::string o;
    for (char c : s) if (!has(o, c)) o.push_back(c);
    return o;
}
inline bool is_ws(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\f'; }
inline std::string strip_ws(const std::string &s) {
    std::string o;
    for (char c : s) if (!is_ws(c)) o.push_back(c);
    return o;
}
inline bool valid_term(const std::string &t) { // is_valid_term, einsum_parser.rs:231-237
    const size_t e = t.find("...");
    std::string letters = t;
    if (e != std::string::npos) {
        if (t.find("...", e + 3) != std::string::npos) return false;
        letters = t.substr(0, e) + t.substr(e + 3);
    }
    for (char c : letters) if (!((c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z'))) return false;
    return true;
}

// EinsumExpr::parse, einsum_parser.rs:68-103
inline void parse_equation(const std::string &equation, std::vector<std::string> &terms, std::string &out) {
    const size_t arrow = equation.find("->");
    const std::string lhs = equation.substr(0, arrow);
    terms.clear();
    size_t b = 0;
    for (;;) {
        const size_t c = lhs.find(',', b);
        terms.push_back(strip_ws(lhs.substr(b, c == std::string::npos ? c : c - b)));
        if (c == std::string::npos) break;
        b = c + 1;
    }
    for (auto &t : terms) if (!valid_term(t)) throw OpError(OpError::InvalidValue, "Input term is invalid");
    if (arrow != std::string::npos) out = strip_ws(equation.substr(arrow + 2));
    else { // default_output, :191-228: "..." then the letters used exactly once, in ASCII order
        int count[128] = {0};
        bool dots = false;
        for (auto &t : terms) { dots = dots || t.find("...") != std::string::npos; for (char c : t) if (c != '.') count[(int)c]++; }
        out = dots ? "..." : "";
        for (int c = 0; c < 128; c++) if (count[c] == 1) out.push_back((char)c);
    }
    if (!valid_term(out)) throw OpError(OpError::InvalidValue, "Output term is invalid");
    for (size_t i = 0; i < out.size(); i++)
        if (out[i] != '.' && out.find(out[i], i + 1) != std::string::npos) throw OpError(OpError::InvalidValue, "Einsum output term contains repeated labels");
    for (char c : out) {
        if (c == '.') continue;
        bool found = false;
        for (auto &t : terms) found = found || has(t, c);
        if (!found) throw OpError(OpError::InvalidValue, "Einsum output term contains a label not present in any input term");
    }
}

// EinsumExpr::validate_inputs (einsum_parser.rs:109-165) with the error mapping of einsum.rs:69-86
inline int broadcast_ndim(const std::vector<std::string> &terms, const std::vector<int> &ndims) {
    if (ndims.size() != terms.size()) throw OpError(OpError::InvalidValue, "Number of terms in Einsum equation does not match input tensor count");
    int b = -1;
    for (size_t i = 0; i < terms.size(); i++) {
        const bool dots = terms[i].find("...") != std::string::npos;
        const int named = (int)terms[i].size() - (dots ? 3 : 0), nd = ndims[i];
        if (dots ? nd < named : nd != named) throw OpError(OpError::InvalidValue, "Einsum term dimension count does not match input tensor");
        if (nd > MAX_DIMS) throw OpError(OpError::UnsupportedValue, "Einsum input or term has too many dimensions");
        if (dots) {
            if (b >= 0 && b != nd - named) throw OpError(OpError::InvalidValue, "Number of broadcast dims does not match across inputs");
            b = nd - named;
        }
    }
    return b < 0 ? 0 : b;
}

inline std::string expand_ellipsis(const std::string &t, int n) { // einsum_parser.rs:254-265
    const size_t e = t.find("...");
    if (e == std::string::npos) return t;
    std::string digits;
    for (int i = 0; i < n; i++) digits.push_back((char)('0' + i));
    return t.substr(0, e) + digits + t.substr(e + 3);
}

struct Step { // EinsumStep, einsum.rs:558-564; a source is an input index or -1 for the previous step's result
    std::string lhs;
    int lhs_src = 0;
    bool binary = false;
    std::string rhs;
    int rhs_src = 0;
    std::string out;
};

// einsum_path, einsum.rs:605-692
inline std::vector<Step> plan_path(std::vector<std::string> terms, std::string out, int bdims) {
    out = expand_ellipsis(out, bdims);
    for (auto &t : terms) t = expand_ellipsis(t, bdims);
    std::vector<Step> steps;
    if (terms.size() <= 2) {
        Step s;
        s.lhs = terms[0]; s.binary = terms.size() == 2; s.out = out;
        if (s.binary) { s.rhs = terms[1]; s.rhs_src = 1; }
        steps.push_back(s);
        return steps;
    }
    std::map<char, int> pending; // reduced label -> terms that still have to consume it
    for (auto &t : terms) for (char c : dedup(t)) if (!has(out, c)) pending[c]++;
    auto consume = [&](const std::string &t) { for (char c : dedup(t)) if (pending.count(c)) pending[c]--; };
    auto keep = [&](const std::string &a, const std::string &b) {
        std::string o;
        for (char c : dedup(a + b)) if (has(out, c) || (pending.count(c) && pending[c] > 0)) o.push_back(c);
        return o;
    };
    consume(terms[0]);
    consume(terms[1]);
    std::string cur = keep(terms[0], terms[1]);
    Step first;
    first.lhs = terms[0]; first.binary = true; first.rhs = terms[1]; first.rhs_src = 1; first.out = cur;
    steps.push_back(first);
    for (size_t i = 2; i < terms.size(); i++) {
        consume(terms[i]);
        const std::string nxt = i + 1 == terms.size() ? out : keep(cur, terms[i]);
        Step s;
        s.lhs = cur; s.lhs_src = -1; s.binary = true; s.rhs = terms[i]; s.rhs_src = (int)i; s.out = nxt;
        steps.push_back(s);
        cur = nxt;
    }
    return steps;
}

struct View {
    const float *p = nullptr;
    Shape shape, strides;
    static View of(const Tensor &t) {
        View v;
        v.p = (const float *)t.ptr();
        v.shape = t.shape();
        v.strides.assign(v.shape.size(), 0);
        int64_t acc = 1;
        for (int d = (int)v.shape.size() - 1; d >= 0; d--) { v.strides[(size_t)d] = acc; acc *= v.shape[(size_t)d]; }
        return v;
    }
    int nd() const { return (int)shape.size(); }
    int64_t len() const { return detail::prod(shape, 0, shape.size()); }
    View relabel(const std::string &have, const std::string &want) const { // permute_and_insert_axes, einsum.rs:414-442
        View v;
        v.p = p;
        for (char c : want) {
            const size_t i = have.find(c);
            v.shape.push_back(i == std::string::npos ? 1 : shape[i]);
            v.strides.push_back(i == std::string::npos ? 0 : strides[i]);
        }
        return v;
    }
    View expanded(const Shape &to) const {
        View v = *this;
        for (size_t i = 0; i < to.size(); i++) if (shape[i] == 1 && to[i] != 1) v.strides[i] = 0;
        v.shape = to;
        return v;
    }
};

// drops 1-sized axes and merges neighbours (outer, inner) with outer stride == inner stride * inner size in every operand
inline void merge_axes(const Shape &shape, const std::vector<Shape> &strides, Shape &mshape, std::vector<Shape> &mstrides) {
    mshape.clear();
    mstrides.assign(strides.size(), Shape());
    for (size_t i = 0; i < shape.size(); i++) {
        if (shape[i] == 1) continue;
        bool merge = !mshape.empty();
        for (size_t k = 0; merge && k < strides.size(); k++) merge = mstrides[k].back() == strides[k][i] * shape[i];
        if (merge) { mshape.back() *= shape[i]; for (size_t k = 0; k < strides.size(); k++) mstrides[k].back() = strides[k][i]; }
        else { mshape.push_back(shape[i]); for (size_t k = 0; k < strides.size(); k++) mstrides[k].push_back(strides[k][i]); }
    }
}
inline Shape broadcast(const Shape &a, const Shape &b, const char *msg) {
    Shape o(a.size());
    for (size_t i = 0; i < a.size(); i++) {
        if (a[i] != b[i] && a[i] != 1 && b[i] != 1) throw OpError(OpError::IncompatibleInputShapes, msg);
        o[i] = a[i] == 1 ? b[i] : a[i];
    }
    return o;
}

inline Tensor materialize(Context &ctx, const View &v, DType dt = DType::F32) { // to_tensor / to_contiguous / expand_to (any 4-byte element type)
    Tensor y(ctx, v.shape, dt);
    if (y.len()) {
        Shape ms; std::vector<Shape> mst;
        merge_axes(v.shape, {v.strides}, ms, mst);
        if (ms.size() > 6) throw OpError(OpError::UnsupportedValue, "Einsum view with more than 6 non-mergeable dims is not supported by the device path");
        ctx.check(rten_hip_copy_strided_b32(ctx.raw(), (int)ms.size(), ms.data(), mst[0].data(), v.p, y.ptr()));
    }
    return y;
}

// The dims of `v` outside `axes` (kept: `kshape`) and inside (reduced) as the merged shape + stride lists the strided reductions' ABI takes.  mos[0] and
// mis[0] are v's own strides; mos[1 + k] are the kept dims' strides in `others[k]`, a full-rank stride list of another view of v's shape (TopK's outputs),
// and kept dims merge only where every list agrees.  `too_many`: the refusal of more than 6 levels; nullptr leaves that to the caller.
struct Split { Shape kshape, mo, mi; std::vector<Shape> mos, mis; };
inline Split split_dims(const View &v, const std::vector<int> &axes, const std::vector<Shape> &others = {},
                        const char *too_many = "more than 6 non-mergeable dims are not supported by the device path") {
    Split r;
    Shape rs, rst;
    std::vector<Shape> kst(1 + others.size());
    for (size_t d = 0; d < v.shape.size(); d++) {
        if (std::find(axes.begin(), axes.end(), (int)d) != axes.end()) { rs.push_back(v.shape[d]); rst.push_back(v.strides[d]); continue; }
        r.kshape.push_back(v.shape[d]);
        kst[0].push_back(v.strides[d]);
        for (size_t k = 0; k < others.size(); k++) kst[k + 1].push_back(others[k][d]);
    }
    merge_axes(r.kshape, kst, r.mo, r.mos);
    merge_axes(rs, {rst}, r.mi, r.mis);
    if (too_many && (r.mo.size() > 6 || r.mi.size() > 6)) throw OpError(OpError::UnsupportedValue, too_many);
    return r;
}

// reduce_sum(view, axes, keep_dims = false): axes sorted and unique
inline Tensor reduce_sum(Context &ctx, const View &v, const std::vector<int> &axes, bool mean = false) {
    const Split d = split_dims(v, axes, {}, nullptr);
    Tensor y(ctx, d.kshape, DType::F32);
    if (y.len()) {
        if (d.mo.size() > 6 || d.mi.size() > 6) throw OpError(OpError::UnsupportedValue, "Einsum reduction over more than 6 non-mergeable dims is not supported by the device path");
        ctx.check((mean ? rten_hip_reduce_mean_strided_f32 : rten_hip_reduce_sum_strided_f32)(ctx.raw(), (int)d.mo.size(), d.mo.data(), d.mos[0].data(), (int)d.mi.size(), d.mi.data(), d.mis[0].data(), v.p, (float *)y.ptr()));
    }
    return y;
}

inline Tensor mul(Context &ctx, const View &a, const View &b) { // mul() with numpy broadcasting on views of equal rank
    const Shape shape = broadcast(a.shape, b.shape, "Cannot broadcast inputs");
    Tensor y(ctx, shape, DType::F32);
    if (y.len()) {
        Shape ms; std::vector<Shape> mst;
        merge_axes(shape, {a.expanded(shape).strides, b.expanded(shape).strides}, ms, mst);
        if (ms.size() > 6) throw OpError(OpError::UnsupportedValue, "broadcasting over more than 6 dims is not supported by the device path");
        ctx.check(rten_hip_binary_broadcast_f32(ctx.raw(), 1, (int)ms.size(), ms.data(), mst[0].data(), mst[1].data(), a.p, b.p, (float *)y.ptr()));
    }
    return y;
}

// matmul() of [batch.., M, K] x [batch.., K, N] views of equal rank, src/ops/matmul.rs:208-385
// `into`: [batch.., M, N] view (N contiguous) of the caller's output tensor; the GEMM then writes the permuted output directly
// through ldc and the C batch strides.  Returns false when those strides do not fit the descriptor's two batch levels.
inline bool matmul_into(Context &ctx, View a, View b, const View &cv) {
    const int nd = a.nd();
    const int64_t m = a.shape[(size_t)nd - 2], k = a.shape[(size_t)nd - 1], n = b.shape[(size_t)nd - 1];
    if (k != b.shape[(size_t)nd - 2]) throw OpError(OpError::IncompatibleInputShapes, "Columns of first matrix does not match rows of second matrix");
    const Shape apre(a.shape.begin(), a.shape.end() - 2), bpre(b.shape.begin(), b.shape.end() - 2);
    const Shape pre = broadcast(apre, bpre, "Cannot broadcast shapes");
    float *const c = const_cast<float *>(cv.p);
    if (cv.len() == 0) return true;
    if (k == 0) { ctx.check(rten_hip_memset(ctx.raw(), c, 0, (size_t)cv.len() * 4)); return true; } // the output tensor is exactly this view's elements
    std::vector<Tensor> keep; // re-laid operands stay alive until the launch is enqueued
    auto relay = [&](View &v) { keep.push_back(materialize(ctx, v)); v = View::of(keep.back()); };
    auto gemm_axis_is_broadcast = [&](const View &v) {
        for (int d = nd - 2; d < nd; d++) if (v.strides[(size_t)d] == 0 && v.shape[(size_t)d] > 1) return true;
        return false;
    };
    if (gemm_axis_is_broadcast(a)) relay(a); // expand_dim, einsum.rs:210-223
    if (gemm_axis_is_broadcast(b)) relay(b);
    rten_hip_gemm_desc d;
    std::memset(&d, 0, sizeof d);
    d.n = (int32_t)n; d.k = (int32_t)k; d.ldc = std::max(cv.strides[(size_t)nd - 2], n); d.alpha = 1.0f; d.batch = 1;
    const int64_t na = detail::prod(apre, 0, apre.size()), nb = detail::prod(bpre, 0, bpre.size());
    Shape ms; std::vector<Shape> mst;
    Shape crows_shape = pre, crows, crows_strides(cv.strides.begin(), cv.strides.end() - 1);
    crows_shape.push_back(m);
    std::vector<Shape> crows_st;
    merge_axes(crows_shape, {crows_strides}, crows, crows_st);
    if (na > 1 && nb == 1 && crows.size() <= 1) { // [A, M, K] x [K, N] as one GEMM of A * M rows (matmul.rs:266-297)
        auto rows = [&] { merge_axes(Shape(a.shape.begin(), a.shape.end() - 1), {Shape(a.strides.begin(), a.strides.end() - 1)}, ms, mst); };
        rows();
        if (ms.size() > 1) { relay(a); rows(); }
        d.m = (int32_t)(na * m);
        d.a_rs = ms.empty() ? 0 : mst[0][0]; d.a_cs = a.strides[(size_t)nd - 1];
        d.b_rs = b.strides[(size_t)nd - 2]; d.b_cs = b.strides[(size_t)nd - 1];
        d.ldc = crows.empty() ? n : std::max(crows_st[0][0], n);
        ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, a.p, b.p, nullptr, c));
        return true;
    }
    Shape ea_shape = pre, eb_shape = pre;
    ea_shape.push_back(m); ea_shape.push_back(k);
    eb_shape.push_back(k); eb_shape.push_back(n);
    View ea = a.expanded(ea_shape), eb = b.expanded(eb_shape);
    auto batch_strides = [&](const View &v) { return Shape(v.strides.begin(), v.strides.end() - 2); };
    merge_axes(pre, {batch_strides(ea), batch_strides(eb), batch_strides(cv)}, ms, mst);
    if (ms.size() > 2) { // more batch levels than the descriptor has: re-lay the operand(s) that do not merge by themselves
        auto needs_relay = [&](const View &v) {
            Shape s1; std::vector<Shape> st1;
            merge_axes(pre, {batch_strides(v)}, s1, st1);
            return s1.size() > 1 || (!st1[0].empty() && st1[0][0] == 0);
        };
        if (needs_relay(ea)) relay(ea);
        if (needs_relay(eb)) relay(eb);
        merge_axes(pre, {batch_strides(ea), batch_strides(eb), batch_strides(cv)}, ms, mst);
        if (ms.size() > 2) return false; // only a permuted C can still refuse to merge: the caller multiplies, then copies
    }
    d.m = (int32_t)m;
    d.a_rs = ea.strides[(size_t)nd - 2]; d.a_cs = ea.strides[(size_t)nd - 1];
    d.b_rs = eb.strides[(size_t)nd - 2]; d.b_cs = eb.strides[(size_t)nd - 1];
    d.batch = (int32_t)detail::prod(ms, 0, ms.size());
    if (ms.size() == 2) {
        d.a_bs = mst[0][0]; d.b_bs = mst[1][0]; d.c_bs = mst[2][0];
        d.batch_inner = (int32_t)ms[1]; d.a_bsi = mst[0][1]; d.b_bsi = mst[1][1]; d.c_bsi = mst[2][1];
    } else if (ms.size() == 1) {
        d.a_bs = mst[0][0]; d.b_bs = mst[1][0]; d.c_bs = mst[2][0];
    }
    ctx.check(rten_hip_gemm_f32(ctx.raw(), &d, ea.p, eb.p, nullptr, c));
    return true;
}
inline Tensor matmul(Context &ctx, const View &a, const View &b) {
    const int nd = a.nd();
    Shape oshape = broadcast(Shape(a.shape.begin(), a.shape.end() - 2), Shape(b.shape.begin(), b.shape.end() - 2), "Cannot broadcast shapes");
    oshape.push_back(a.shape[(size_t)nd - 2]);
    oshape.push_back(b.shape[(size_t)nd - 1]);
    Tensor y(ctx, oshape, DType::F32);
    matmul_into(ctx, a, b, View::of(y)); // a contiguous C always fits
    return y;
}

inline View diagonals(std::string &term, const View &v) { // take_diagonals, einsum.rs:124-162
    const std::string labels = dedup(term);
    View o;
    o.p = v.p;
    for (char c : labels) {
        int64_t size = -1, stride = 0;
        for (size_t i = 0; i < term.size(); i++) {
            if (term[i] != c) continue;
            if (size >= 0 && v.shape[i] != size) throw OpError(OpError::InvalidValue, "Dimension sizes for repeated labels in term do not match");
            size = v.shape[i];
            stride += v.strides[i];
        }
        o.shape.push_back(size);
        o.strides.push_back(stride);
    }
    term = labels;
    return o;
}

inline int64_t bsize(int64_t a, int64_t b) { // broadcast_size, einsum.rs:197-205
    if (a == b || b == 1) return a;
    if (a == 1) return b;
    throw OpError(OpError::IncompatibleInputShapes, "Einsum label has different sizes in different terms");
}

// einsum_matmul, einsum.rs:449-537
inline Tensor contract(Context &ctx, const View &x, const View &y, const std::string &tx, const std::string &ty, const std::string &out, char kl) {
    char nl = INS_N, ml = INS_M;
    for (size_t i = ty.size(); i-- > 0;) if (!has(tx, ty[i])) { nl = ty[i]; break; }
    for (size_t i = tx.size(); i-- > 0;) if (!has(ty, tx[i])) { ml = tx[i]; break; }
    std::string batch;
    for (char c : dedup(tx + ty)) if (c != kl && c != ml && c != nl) batch.push_back(c);
    View xv = x.relabel(tx, batch + ml + kl), yv = y.relabel(ty, batch + kl + nl);
    const int64_t ks = bsize(xv.shape.back(), yv.shape[yv.shape.size() - 2]);
    Shape xs = xv.shape, ys = yv.shape;
    xs.back() = ks;
    ys[ys.size() - 2] = ks;
    const std::string full = batch + ml + nl;
    std::string order;
    for (char c : full) if (c != INS_M && c != INS_N) order.push_back(c);
    if (order != out && (nl == INS_N || out.back() == nl)) {
        // the output permutation keeps N innermost: the GEMM writes the permuted tensor directly (C strides), no copy
        Shape fshape;
        for (char c : out) {
            const size_t i = full.find(c);
            fshape.push_back(i + 2 == full.size() ? xs[xs.size() - 2] : i + 1 == full.size() ? ys.back() : (xs[i] == 1 ? ys[i] : xs[i]));
        }
        Tensor final(ctx, fshape, DType::F32);
        if (matmul_into(ctx, xv.expanded(xs), yv.expanded(ys), View::of(final).relabel(out, full))) return final;
    }
    Tensor r = matmul(ctx, xv.expanded(xs), yv.expanded(ys));
    Shape shape;
    for (size_t i = 0; i < full.size(); i++) if (full[i] != INS_M && full[i] != INS_N) shape.push_back(r.size((int)i));
    r.reshape(shape);
    if (order == out) return r;
    return materialize(ctx, View::of(r).relabel(order, out));
}

// einsum_step, einsum.rs:238-364
inline Tensor run_step(Context &ctx, const Step &s, View x, const View *yin) {
    std::string tx = s.lhs, ty = s.rhs;
    const std::string &out = s.out;
    x = diagonals(tx, x);
    auto reduced = [&](const std::string &labels) { std::string r; for (char c : labels) if (!has(out, c)) r.push_back(c); return r; };
    auto trailing = [&](size_t from, size_t count) { std::vector<int> a; for (size_t i = 0; i < count; i++) a.push_back((int)(from + i)); return a; };
    if (!s.binary) {
        const std::string red = reduced(tx);
        const View xv = x.relabel(tx, out + red);
        return red.empty() ? materialize(ctx, xv) : reduce_sum(ctx, xv, trailing(out.size(), red.size()));
    }
    View y = diagonals(ty, *yin);
    std::vector<Tensor> keep;
    auto drop_lone = [&](View &v, std::string &term, const std::string &other) { // sum_lone_dims, einsum.rs:168-190
        std::vector<int> lone;
        std::string kept;
        for (size_t i = 0; i < term.size(); i++) {
            if (has(other, term[i]) || has(out, term[i])) kept.push_back(term[i]);
            else lone.push_back((int)i);
        }
        if (!lone.empty()) { keep.push_back(reduce_sum(ctx, v, lone)); v = View::of(keep.back()); }
        term = kept;
    };
    drop_lone(x, tx, ty);
    drop_lone(y, ty, tx);
    const std::string red = reduced(dedup(tx + ty));
    if (red.size() == 1) return contract(ctx, x, y, tx, ty, out, red[0]);
    const View xv = x.relabel(tx, out + red), yv = y.relabel(ty, out + red);
    if (red.empty()) return mul(ctx, xv, yv);
    Shape xs = xv.shape, ys = yv.shape; // several reduced labels: re-laid side by side and merged into one K (einsum.rs:310-344)
    int64_t ksz = 1;
    for (size_t i = out.size(); i < xs.size(); i++) { xs[i] = ys[i] = bsize(xs[i], ys[i]); ksz *= xs[i]; }
    Tensor xc = materialize(ctx, xv.expanded(xs)), yc = materialize(ctx, yv.expanded(ys));
    xs.resize(out.size()); xs.push_back(ksz);
    ys.resize(out.size()); ys.push_back(ksz);
    xc.reshape(xs);
    yc.reshape(ys);
    return contract(ctx, View::of(xc), View::of(yc), out + MERGED_K, out + MERGED_K, out, MERGED_K);
}
} // namespace einsum_detail

// ------------------------------------------------------------------------------------------------ Reduce* and selection families
// ReduceSum / ReduceMean (src/ops/reduce.rs:523-580, 1126-1165), ReduceMax / ReduceMin / ArgMax / ArgMin / TopK (:64-215, 876-1044, 1236-1356) and the six
// kinds of rten_hip_reduce_strided.  ReduceSum is float32; the selection family takes float32 and int32 tensors; index outputs are int32.  The kernels
// (rten_amd/csrc/reduce.hip, select.hip) read the view in place through its strides and never report back to the host.
namespace select_detail {
inline int32_t abi_dtype(const Tensor &x) { // map_value_view!(.., [FloatTensor, Int32Tensor], ..)
    if (x.dtype() == DType::F32) return RTEN_HIP_DT_F32;
    if (x.dtype() == DType::I32) return RTEN_HIP_DT_I32;
    throw OpError(OpError::UnsupportedType, "");
}
// an int32 operand the host reads (axes, K): its host copy when it has one, a read-back otherwise (a graph executor refuses that case before it gets here)
inline std::vector<int64_t> host_ints(const Tensor &t) {
    want(t, DType::I32, "int32");
    if (t.host()) return t.host()->i;
    std::vector<int64_t> v;
    for (int32_t e : t.to_host<int32_t>()) v.push_back(e);
    return v;
}
// one value of type `out` per slice of `v` over the sorted unique axes `ax`, shaped as the kept dims; `launch(split, y)` calls the entry point
template <class Launch>
inline Tensor reduce_slices(Context &ctx, const einsum_detail::View &v, const std::vector<int> &ax, DType out, Launch launch) {
    const einsum_detail::Split d = einsum_detail::split_dims(v, ax);
    Tensor y(ctx, d.kshape, out);
    if (y.len()) ctx.check(launch(d, y.ptr()));
    return y;
}
// keep_dims: the reduced dims `ax` of `shape` come back with size 1
inline void restore_kept_dims(Tensor &y, std::vector<int64_t> shape, const std::vector<int> &ax) {
    for (int a : ax) shape[(size_t)a] = 1;
    y.reshape(shape);
}
} // namespace select_detail

// What the operators of reduce() (src/ops/reduce.rs:414-520) do differently around ReduceOp::run, each as the reference has it
struct ReduceRules {
    bool axes_input;  // a second input replaces the `axes` attribute.  Not ReduceSum / ReduceMean: theirs is resolved into the attribute by the graph executor
    bool int32;       // Int32Tensor is taken too (the generic kernels: wrapping arithmetic, or a comparison)
    bool typed_first; // the operand's type is checked before noop_with_empty_axes is looked at (map_value_view! / require_as outside the test,
                      // reduce.rs:687,752,827,1215); otherwise only a reduction that runs checks it
    bool cast_error;  // float32 only through require_as (its cast error) rather than map_value_view! (UnsupportedType)
    enum Skipped { Copy, Abs, Square, Ln } skipped; // noop_with_empty_axes and no axes: the element map still applies -- x, |x| (reduce.rs:828-830),
                                                    // x * x (:1216-1218), ln x (:688-690)
    enum Rank0 { CopyUnchecked, CopyChecked, SliceOfOne } rank0; // a 0-d input: itself, without looking at the axes; itself, after the axes were
                                                                 // validated (reduce.rs:425-428); the kernel's value for a slice of one element
};

struct ReduceOp : Operator {
    std::vector<int> axes;
    bool keep_dims = true, noop_with_empty_axes = false;
    int max_inputs() const override { return 2; }
    virtual ReduceRules rules() const = 0;
    // one value per slice of `v` (a view of all of `x`) over the sorted unique axes `ax`, shaped as the kept dims
    virtual Tensor reduce(Context &ctx, const Tensor &x, const einsum_detail::View &v, const std::vector<int> &ax) const = 0;
    OutputList run(Context &ctx, const InputList &in) const override {
        namespace E = einsum_detail;
        const ReduceRules r = rules();
        const Tensor &x = require(in, 0);
        std::vector<int> given = axes;
        if (const Tensor *a = r.axes_input ? get(in, 1) : nullptr) { given.clear(); for (int64_t e : select_detail::host_ints(*a)) given.push_back((int)e); }
        auto check_type = [&] {
            if (x.dtype() == DType::F32 || (r.int32 && x.dtype() == DType::I32)) return;
            if (r.cast_error) want(x, DType::F32, "float32");
            throw OpError(OpError::UnsupportedType, "");
        };
        if (r.typed_first) check_type();
        const E::View v = E::View::of(x);
        OutputList out;
        if (given.empty() && noop_with_empty_axes) {
            if (dtype_size(x.dtype()) != 4) throw OpError(OpError::UnsupportedType, "");
            InputList self{&x};
            if (r.skipped == ReduceRules::Abs) return Abs().run(ctx, self);
            if (r.skipped == ReduceRules::Ln) return Log().run(ctx, self);
            if (r.skipped == ReduceRules::Square) out.push_back(broadcast_binary(ctx, x, x, 1, RTEN_HIP_EW_IMUL));
            else out.push_back(E::materialize(ctx, v, x.dtype()));
            return out;
        }
        check_type();
        const int nd = x.ndim();
        if (nd == 0) {
            if (r.rank0 != ReduceRules::CopyUnchecked) for (int a : given) resolve_axis(a, 0);
            if (r.rank0 != ReduceRules::SliceOfOne) { out.push_back(E::materialize(ctx, v, x.dtype())); return out; }
        }
        const std::vector<int> ax = nd ? resolve_axes(given, nd) : std::vector<int>();
        Tensor y = reduce(ctx, x, v, ax);
        if (keep_dims) select_detail::restore_kept_dims(y, x.shape(), ax);
        out.push_back(std::move(y));
        return out;
    }
};

struct ReduceSum : ReduceOp { // src/ops/reduce.rs:1126-1165 (f32)
    bool mean = false;
    const char *name() const override { return mean ? "ReduceMean" : "ReduceSum"; }
    ReduceRules rules() const override { return {false, false, true, true, ReduceRules::Copy, ReduceRules::CopyUnchecked}; }
    Tensor reduce(Context &ctx, const Tensor &, const einsum_detail::View &v, const std::vector<int> &ax) const override { return einsum_detail::reduce_sum(ctx, v, ax, mean); }
};
struct ReduceMean : ReduceSum { // src/ops/reduce.rs:523-580: Sum / len per slice
    ReduceMean() { mean = true; }
};

struct ReduceMax : ReduceOp { // src/ops/reduce.rs:977-1044
    bool min = false;
    const char *name() const override { return min ? "ReduceMin" : "ReduceMax"; }
    ReduceRules rules() const override { return {true, true, true, false, ReduceRules::Copy, ReduceRules::CopyChecked}; }
    Tensor reduce(Context &ctx, const Tensor &x, const einsum_detail::View &v, const std::vector<int> &ax) const override {
        return select_detail::reduce_slices(ctx, v, ax, x.dtype(), [&](const einsum_detail::Split &d, void *y) {
            return rten_hip_reduce_minmax_strided(ctx.raw(), min ? RTEN_HIP_SELECT_MIN : RTEN_HIP_SELECT_MAX, select_detail::abi_dtype(x), (int)d.mo.size(), d.mo.data(),
                                                  d.mos[0].data(), (int)d.mi.size(), d.mi.data(), d.mis[0].data(), v.p, y);
        });
    }
};
struct ReduceMin : ReduceMax { // src/ops/reduce.rs:907-975
    ReduceMin() { min = true; }
};

// ReduceL1 / ReduceSumSquare / ReduceL2 / ReduceLogSum / ReduceLogSumExp / ReduceProd (src/ops/reduce.rs:590-845, 1046-1100, 1167-1234) around one kernel
// of rten_hip_reduce_strided (rten_amd/csrc/reduce.hip); an empty slice gives the kernel's value for it.
struct Reduce : ReduceOp {
    int kind;
    const char *nm;
    bool int32, typed_first, cast_error; // as ReduceRules has them
    Reduce(int k, const char *n, bool i32, bool tf, bool ce) : kind(k), nm(n), int32(i32), typed_first(tf), cast_error(ce) {}
    const char *name() const override { return nm; }
    ReduceRules rules() const override {
        const ReduceRules::Skipped skipped = kind == RTEN_HIP_REDUCE_L1 ? ReduceRules::Abs : kind == RTEN_HIP_REDUCE_SUM_SQUARE ? ReduceRules::Square
                                             : kind == RTEN_HIP_REDUCE_LOG_SUM ? ReduceRules::Ln : ReduceRules::Copy;
        return {true, int32, typed_first, cast_error, skipped, ReduceRules::SliceOfOne};
    }
    Tensor reduce(Context &ctx, const Tensor &x, const einsum_detail::View &v, const std::vector<int> &ax) const override {
        return select_detail::reduce_slices(ctx, v, ax, x.dtype(), [&](const einsum_detail::Split &d, void *y) {
            return rten_hip_reduce_strided(ctx.raw(), kind, select_detail::abi_dtype(x), (int)d.mo.size(), d.mo.data(), d.mos[0].data(), (int)d.mi.size(), d.mi.data(),
                                           d.mis[0].data(), v.p, y);
        });
    }
};
struct ReduceL1 : Reduce { ReduceL1() : Reduce(RTEN_HIP_REDUCE_L1, "ReduceL1", true, true, false) {} };                             // reduce.rs:775-845
struct ReduceSumSquare : Reduce { ReduceSumSquare() : Reduce(RTEN_HIP_REDUCE_SUM_SQUARE, "ReduceSumSquare", true, true, false) {} }; // reduce.rs:1167-1234
struct ReduceL2 : Reduce { ReduceL2() : Reduce(RTEN_HIP_REDUCE_L2, "ReduceL2", false, false, false) {} };                            // reduce.rs:590-651
struct ReduceLogSum : Reduce { ReduceLogSum() : Reduce(RTEN_HIP_REDUCE_LOG_SUM, "ReduceLogSum", false, true, true) {} };             // reduce.rs:653-708
struct ReduceLogSumExp : Reduce { ReduceLogSumExp() : Reduce(RTEN_HIP_REDUCE_LOG_SUM_EXP, "ReduceLogSumExp", false, true, true) {} }; // reduce.rs:710-773
struct ReduceProd : Reduce { ReduceProd() : Reduce(RTEN_HIP_REDUCE_PROD, "ReduceProd", true, false, false) {} };                     // reduce.rs:1046-1100

// LpNormalization (src/ops/norm.rs:611-693): every lane along `axis` times 1 / norm, norm = SumAbs (p = 1) or sqrt(SumSquare) (p = 2); a zero norm zeroes
// the lane.  Defaults as the reference's loader (onnx_registry.rs:1284-1287).  Lanes along a non-last axis are read and written through the axis stride.
struct LpNormalization : Operator {
    int axis = -1, p = 2;
    const char *name() const override { return "LpNormalization"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        namespace E = einsum_detail;
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        if (p != 1 && p != 2) throw OpError(OpError::UnsupportedValue, "`p` must be 1 or 2");
        const int a = resolve_axis(axis, x.ndim());
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len()) {
            const E::View v = E::View::of(x);
            const E::Split d = E::split_dims(v, {a});
            ctx.check(rten_hip_lp_normalize_f32(ctx.raw(), p, (int)d.mo.size(), d.mo.data(), d.mos[0].data(), v.shape[(size_t)a], v.strides[(size_t)a], v.p, (float *)y.ptr()));
        }
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

// GlobalMaxPool (src/ops/pooling.rs:477-514,549-580): MaxNum over dims 2.. of an input of at least 2 dims, output [N, C, 1, ...]
struct GlobalMaxPool : Operator {
    const char *name() const override { return "GlobalMaxPool"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        namespace E = einsum_detail;
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        if (x.ndim() < 2) throw OpError(OpError::InvalidValue, "Input must have at least 2 dims");
        std::vector<int> ax;
        for (int d = 2; d < x.ndim(); d++) ax.push_back(d);
        const E::View v = E::View::of(x);
        Tensor y = select_detail::reduce_slices(ctx, v, ax, DType::F32, [&](const E::Split &d, void *yp) {
            return rten_hip_reduce_minmax_strided(ctx.raw(), RTEN_HIP_SELECT_MAX, RTEN_HIP_DT_F32, (int)d.mo.size(), d.mo.data(), d.mos[0].data(), (int)d.mi.size(), d.mi.data(),
                                                  d.mis[0].data(), v.p, yp);
        });
        select_detail::restore_kept_dims(y, x.shape(), ax);
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

struct ArgMax : Operator { // src/ops/reduce.rs:64-160: the FIRST NaN of a lane that holds one, otherwise the LAST element equal to the extreme
    int axis = 0;
    bool keep_dims = true, min = false;
    const char *name() const override { return min ? "ArgMin" : "ArgMax"; }
    int max_inputs() const override { return 1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        namespace E = einsum_detail;
        namespace S = select_detail;
        const Tensor &x = require(in, 0);
        const int32_t dt = S::abi_dtype(x);
        const int a = resolve_axis(axis, x.ndim());
        if (x.size(a) == 0) throw OpError(OpError::InvalidValue, "Cannot select index from empty sequence");
        const E::View v = E::View::of(x);
        Tensor y = S::reduce_slices(ctx, v, {a}, DType::I32, [&](const E::Split &d, void *yp) {
            return rten_hip_arg_minmax_strided(ctx.raw(), min ? RTEN_HIP_SELECT_MIN : RTEN_HIP_SELECT_MAX, dt, (int)d.mo.size(), d.mo.data(), d.mos[0].data(),
                                               v.shape[(size_t)a], v.strides[(size_t)a], v.p, (int32_t *)yp);
        });
        if (keep_dims) S::restore_kept_dims(y, x.shape(), {a});
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};

struct ArgMin : ArgMax { // src/ops/reduce.rs:162-215
    ArgMin() { min = true; }
};

// TopK (src/ops/reduce.rs:1236-1356): inputs X, K (int32 scalar or one element); outputs values and int32 indices.  NaN is greater than every number
// whatever `largest` says, equal values come by ascending index, the result is always sorted (`sorted` = 0 leaves the order unspecified in the reference).
struct TopK : Operator {
    int axis = -1;
    bool largest = true, sorted = true;
    const char *name() const override { return "TopK"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        namespace E = einsum_detail;
        namespace S = select_detail;
        const Tensor &x = require(in, 0);
        const std::vector<int64_t> kv = S::host_ints(require(in, 1));
        if (kv.size() != 1) throw OpError(OpError::InvalidValue, "Expected scalar value");
        const int64_t k = kv[0];
        if (k < 0) throw OpError(OpError::InvalidValue, "k must be positive");
        const int32_t dt = S::abi_dtype(x);
        const int a = resolve_axis(axis, x.ndim());
        std::vector<int64_t> oshape = x.shape();
        oshape[(size_t)a] = k;
        OutputList out;
        out.emplace_back(ctx, oshape, x.dtype());
        out.emplace_back(ctx, oshape, DType::I32);
        if (k == 0) return out;
        if (k > x.size(a)) throw OpError(OpError::InvalidValue, "k > dimension size");
        if (out[0].len()) {
            const E::View v = E::View::of(x), ov = E::View::of(out[0]);
            const E::Split d = E::split_dims(v, {a}, {ov.strides});
            ctx.check(rten_hip_topk_strided(ctx.raw(), largest ? 1 : 0, dt, (int)d.mo.size(), d.mo.data(), d.mos[0].data(), d.mos[1].data(), v.shape[(size_t)a],
                                            v.strides[(size_t)a], k, v.p, out[0].ptr(), (int32_t *)out[1].ptr(), ov.strides[(size_t)a]));
        }
        return out;
    }
};

struct Einsum : Operator { // src/ops/einsum.rs:21-108
    std::string equation;
    const char *name() const override { return "Einsum"; }
    int max_inputs() const override { return -1; }
    OutputList run(Context &ctx, const InputList &in) const override {
        namespace E = einsum_detail;
        std::vector<int> ndims;
        for (size_t i = 0; i < in.size(); i++) ndims.push_back(want(require(in, i), DType::F32, "float32").ndim());
        std::vector<std::string> terms;
        std::string out;
        E::parse_equation(equation, terms, out);
        const int bdims = E::broadcast_ndim(terms, ndims);
        Tensor result;
        for (const E::Step &s : E::plan_path(terms, out, bdims)) {
            const E::View x = s.lhs_src < 0 ? E::View::of(result) : E::View::of(*in[(size_t)s.lhs_src]);
            E::View y;
            if (s.binary) y = s.rhs_src < 0 ? E::View::of(result) : E::View::of(*in[(size_t)s.rhs_src]);
            Tensor next = E::run_step(ctx, s, x, s.binary ? &y : nullptr);
            result = std::move(next); // the previous result is released only after the step that read it was enqueued
        }
        OutputList o;
        o.push_back(std::move(result));
        return o;
    }
};

// ------------------------------------------------------------------------------------------------ recurrent layers (src/ops/rnn.rs)
enum class RnnDirection { Forward = RTEN_HIP_RNN_FORWARD, Reverse = RTEN_HIP_RNN_REVERSE, Bidirectional = RTEN_HIP_RNN_BIDIRECTIONAL };

namespace rnn_detail {
// static_dims! (src/operator.rs:210-241)
inline const Tensor &dims(const Tensor &t, int nd, const char *what, const char *names = nullptr) {
    if (t.ndim() != nd) throw OpError(OpError::InvalidValue, std::string(what) + " must have " + std::to_string(nd) + " dims" + (names ? " (" + std::string(names) + ")" : ""));
    return want(t, DType::F32, "float32");
}
// Y [seq, dirs, batch, hidden], Y_h (, Y_c) [dirs, batch, hidden]; an output the mask leaves out is an empty Tensor and is not computed
inline OutputList outputs(Context &ctx, const Tensor &x, int64_t hidden, RnnDirection dir, int n_out, unsigned mask) {
    const int64_t dirs = dir == RnnDirection::Bidirectional ? 2 : 1;
    OutputList out;
    for (int i = 0; i < n_out; i++) {
        if (!(mask >> i & 1)) { out.emplace_back(); continue; }
        if (i == 0) out.emplace_back(ctx, std::vector<int64_t>{x.size(0), dirs, x.size(1), hidden}, DType::F32);
        else out.emplace_back(ctx, std::vector<int64_t>{dirs, x.size(1), hidden}, DType::F32);
    }
    return out;
}
} // namespace rnn_detail

// GRU (src/ops/rnn.rs:107-383): inputs X, W, R, B?, sequence_lens? (ignored, as in the reference), initial_h?; gate order update, reset, hidden.
// `output_mask` bit i = compute output i (Y, Y_h): a graph node may leave outputs unnamed.
struct GRU : Operator {
    RnnDirection direction = RnnDirection::Forward;
    int64_t hidden_size = 0; // inferred from W, as in the reference
    bool linear_before_reset = false;
    unsigned output_mask = 3;
    const char *name() const override { return "GRU"; }
    int max_inputs() const override { return 6; }
    OutputList run(Context &ctx, const InputList &in) const override {
        if (!linear_before_reset) throw OpError(OpError::UnsupportedValue, "`linear_before_reset=0` is not supported");
        const Tensor &x = rnn_detail::dims(require(in, 0), 3, "input", "seq, batch, input");
        const Tensor &w = rnn_detail::dims(require(in, 1), 3, "weights", "dir, hidden x 3, input");
        const Tensor &r = rnn_detail::dims(require(in, 2), 3, "recurrent_weights");
        const Tensor *b = get(in, 3), *h0 = get(in, 5);
        if (b) rnn_detail::dims(*b, 2, "bias", "dir, hidden x 6");
        if (h0) rnn_detail::dims(*h0, 3, "initial_hidden");
        const int64_t hidden = w.size(1) / 3;
        OutputList out = rnn_detail::outputs(ctx, x, hidden, direction, 2, output_mask);
        ctx.check(rten_hip_gru_f32(ctx.raw(), (int32_t)x.size(0), (int32_t)x.size(1), (int32_t)x.size(2), (int32_t)hidden, (int32_t)direction, 1, 0, 0, (const float *)x.ptr(), (const float *)w.ptr(), (const float *)r.ptr(), (const float *)vp(b), (const float *)vp(h0),
                                   (float *)out[0].ptr(), (float *)out[1].ptr()));
        return out;
    }
};

// LSTM (src/ops/rnn.rs:385-660): inputs X, W, R, B?, sequence_lens? (ignored), initial_h?, initial_c?; gate order input, output, forget, cell; outputs Y, Y_h, Y_c.
struct LSTM : Operator {
    RnnDirection direction = RnnDirection::Forward;
    int64_t hidden_size = 0;
    unsigned output_mask = 7;
    const char *name() const override { return "LSTM"; }
    int max_inputs() const override { return 7; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = rnn_detail::dims(require(in, 0), 3, "input", "seq, batch, input");
        const Tensor &w = rnn_detail::dims(require(in, 1), 3, "weights", "dir, hidden x 4, input");
        const Tensor &r = rnn_detail::dims(require(in, 2), 3, "recurrent_weights", "dir, hidden x 4, hidden");
        if (w.size(1) % 4 != 0) throw OpError(OpError::InvalidValue, "weights dim 1 must be 4 * hidden_size");
        const Tensor *b = get(in, 3), *h0 = get(in, 5), *c0 = get(in, 6);
        if (b) { rnn_detail::dims(*b, 2, "bias"); if (b->size(1) % 8 != 0) throw OpError(OpError::InvalidValue, "bias dim 1 must be 8 * hidden_size"); }
        if (h0) rnn_detail::dims(*h0, 3, "initial_hidden");
        if (c0) rnn_detail::dims(*c0, 3, "initial_cell");
        const int64_t hidden = w.size(1) / 4;
        OutputList out = rnn_detail::outputs(ctx, x, hidden, direction, 3, output_mask);
        ctx.check(rten_hip_lstm_f32(ctx.raw(), (int32_t)x.size(0), (int32_t)x.size(1), (int32_t)x.size(2), (int32_t)hidden, (int32_t)direction, 0, 0, (const float *)x.ptr(), (const float *)w.ptr(), (const float *)r.ptr(), (const float *)vp(b), (const float *)vp(h0),
                                    (const float *)vp(c0), (float *)out[0].ptr(), (float *)out[1].ptr(), (float *)out[2].ptr()));
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ decoder blocks: RMS / skip normalisation, rotary embedding
namespace decoder_detail {
// `scale.item()` of layer_normalization_impl (src/ops/norm.rs:470): the value of a tensor of exactly one element, whatever its rank.  A constant carries a
// host copy (nothing is read back); a one-element scale that only the device knows is read back, which synchronises.
inline bool one_element(const Tensor &t, float &v) {
    if (t.len() != 1) return false;
    if (t.host() && t.host()->is_float && t.host()->f.size() == 1) v = t.host()->f[0];
    else v = t.to_host<float>()[0];
    return true;
}
// try_broadcast(shape -> target) of rten-tensor: right-aligned, every dim equal or 1, rank not above the target's
inline bool broadcastable(const std::vector<int64_t> &shape, const std::vector<int64_t> &target) {
    if (shape.size() > target.size()) return false;
    for (size_t i = 0; i < shape.size(); i++) {
        const int64_t s = shape[shape.size() - 1 - i], t = target[target.size() - 1 - i];
        if (s != t && s != 1) return false;
    }
    return true;
}
// rotary_cache_dims (src/ops/embedding.rs:20-44): a cos / sin cache is [1 | batch, 1 | seq_len, rotary_embedding_dim / 2]
inline std::pair<int64_t, int64_t> rotary_cache_dims(const std::vector<int64_t> &cache, int64_t batch, int64_t seq_len, int64_t half, const char *bad_last_dim) {
    if (cache.size() != 3) throw OpError(OpError::InvalidValue, "cos/sin cache must be a 3D tensor");
    if (cache[2] != half) throw OpError(OpError::InvalidValue, bad_last_dim);
    if (cache[1] != 1 && cache[1] != seq_len) throw OpError(OpError::InvalidValue, "cos/sin cache sequence length must be 1 or match the input");
    if (cache[0] != 1 && cache[0] != batch) throw OpError(OpError::InvalidValue, "cos/sin cache batch size must be 1 or match the input");
    return {cache[0], cache[1]};
}
// rotary_embedding (src/ops/embedding.rs:46-207) on rten_hip_rotary_embedding_f32.  `ids`: int32 [batch, seq] positions or, with `offset`, the contrib
// operator's one-element offset k (token i uses position k + i).  The kernel gathers the cache rows and reads the offset itself: nothing is read back, no
// intermediate [B, S, half] tensor exists.  Ids the host knows are checked here and refused with Gather's message; ids only the device knows are clamped.
inline Tensor rotary_embedding(Context &ctx, const Tensor &x_in, const Tensor &cos_in, const Tensor &sin_in, const Tensor *ids, bool offset, bool interleaved,
                               int64_t num_heads, int64_t rotary_embedding_dim) {
    const Tensor &x = want(x_in, DType::F32, "float32");
    const Tensor &cos = want(cos_in, DType::F32, "float32"), &sin = want(sin_in, DType::F32, "float32");
    int64_t batch, seq, heads, head_size, st[3];
    if (x.ndim() == 3) {
        if (num_heads == 0) throw OpError(OpError::InvalidValue, "num_heads must not be 0 for 3 dimensioned input");
        if (x.size(2) % num_heads != 0) throw OpError(OpError::InvalidValue, "hidden_size must be divisible by num_heads");
        batch = x.size(0); seq = x.size(1); heads = num_heads; head_size = x.size(2) / num_heads;
        st[0] = seq * x.size(2); st[1] = x.size(2); st[2] = head_size;
    } else if (x.ndim() == 4) {
        batch = x.size(0); heads = x.size(1); seq = x.size(2); head_size = x.size(3);
        st[0] = heads * seq * head_size; st[1] = head_size; st[2] = seq * head_size;
    } else throw OpError(OpError::IncompatibleInputShapes, "Input processed needs 3-4 dimensions");
    const int64_t rot = rotary_embedding_dim == 0 ? head_size : rotary_embedding_dim;
    if (rot == 0 || rot % 2 != 0) throw OpError(OpError::InvalidValue, "rotary_embedding_dim must be a positive even number");
    if (rot > head_size) throw OpError(OpError::InvalidValue, "rotary_embedding_dim must not exceed head size");
    const int64_t half = rot / 2;
    const char *bad_cos = "Last dimension of cos cache does not match rotary_embedding_dim/2", *bad_sin = "Last dimension of sin cache does not match rotary_embedding_dim/2";
    int32_t mode = RTEN_HIP_ROTARY_POS_NONE;
    int64_t max_pos = 0, cst[2] = {0, 0}, sst[2] = {0, 0};
    if (ids) {
        want(*ids, DType::I32, "int32");
        // gather(cache, 0, ids) has the shape ids.shape + cache.shape[1..]
        const std::vector<int64_t> id_shape = offset ? std::vector<int64_t>{batch, seq} : ids->shape();
        for (const Tensor *cache : {&cos, &sin}) {
            if (cache->ndim() == 0) throw OpError(OpError::InvalidValue, "Cannot gather from a scalar");
            std::vector<int64_t> g = id_shape;
            g.insert(g.end(), cache->shape().begin() + 1, cache->shape().end());
            rotary_cache_dims(g, batch, seq, half, cache == &cos ? bad_cos : bad_sin);
        }
        if (cos.size(0) != sin.size(0)) throw OpError(OpError::UnsupportedValue, "device path needs cos and sin caches of one length");
        if (!offset && (ids->size(0) != batch || ids->size(1) != seq)) throw OpError(OpError::UnsupportedValue, "device path needs position_ids of the input's [batch, seq] shape");
        max_pos = cos.size(0);
        if (const HostVal *h = ids->host()) {
            if (!h->is_float)
                for (size_t i = 0; i < h->i.size(); i++) {
                    const int64_t lo = h->i[i], hi = offset ? lo + seq - 1 : lo;
                    if (lo < -max_pos || hi >= max_pos) throw OpError(OpError::InvalidValue, "Entry in `indices` is out of range");
                }
        }
        mode = offset ? RTEN_HIP_ROTARY_POS_OFFSET : RTEN_HIP_ROTARY_POS_IDS;
    } else {
        const auto c = rotary_cache_dims(cos.shape(), batch, seq, half, bad_cos), s = rotary_cache_dims(sin.shape(), batch, seq, half, bad_sin);
        cst[0] = c.first == 1 ? 0 : c.second * half; cst[1] = c.second == 1 ? 0 : half;
        sst[0] = s.first == 1 ? 0 : s.second * half; sst[1] = s.second == 1 ? 0 : half;
    }
    Tensor y(ctx, x.shape(), DType::F32);
    if (x.len())
        ctx.check(rten_hip_rotary_embedding_f32(ctx.raw(), (int32_t)batch, (int32_t)seq, (int32_t)heads, (int32_t)head_size, (int32_t)rot, interleaved ? 1 : 0,
                                                (const float *)x.ptr(), st[0], st[1], st[2], (const float *)cos.ptr(), cst[0], cst[1], (const float *)sin.ptr(), sst[0], sst[1],
                                                (const int32_t *)vp(ids), mode, (int32_t)max_pos, (float *)y.ptr(), st[0], st[1], st[2]));
    return y;
}
} // namespace decoder_detail

// RMSNormalization (src/ops/norm.rs:419-435,571-608; loader defaults onnx_registry.rs:1584-1590: axis -1, epsilon absent = 1e-5, stash_type must be 1).
// inputs X, scale: shape[axis..] is normalised by its root mean square; a one-element scale is the reference's scalar form.
struct RMSNormalization : Operator {
    int axis = -1;
    std::optional<float> epsilon;
    const char *name() const override { return "RMSNormalization"; }
    int max_inputs() const override { return 2; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = want(require(in, 0), DType::F32, "float32");
        const Tensor &scale = want(require(in, 1), DType::F32, "float32");
        const int a = resolve_axis(axis, x.ndim());
        const std::vector<int64_t> norm_shape(x.shape().begin() + a, x.shape().end());
        const int64_t cols = detail::prod(x.shape(), (size_t)a, x.shape().size()), rows = cols ? x.len() / cols : 0;
        float gs = 1.f;
        const bool one = decoder_detail::one_element(scale, gs);
        if (!one) {
            if (!decoder_detail::broadcastable(scale.shape(), norm_shape)) throw OpError(OpError::InvalidValue, "`scale` is not broadcastable to normalized axes of input");
            if (scale.len() != cols) throw OpError(OpError::UnsupportedValue, "device path needs scale already expanded to the normalized shape");
        }
        Tensor y(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_rms_norm_f32(ctx.raw(), rows, (int32_t)cols, (const float *)x.ptr(), one ? nullptr : (const float *)scale.ptr(), gs, epsilon.value_or(1e-5f),
                                            (float *)y.ptr()));
        OutputList out;
        out.push_back(std::move(y));
        return out;
    }
};
// SimplifiedLayerNormalization (src/ops/norm/contrib.rs:86-115): the contrib spelling, registered in ai.onnx (onnx_registry.rs:275,1905)
struct SimplifiedLayerNormalization : RMSNormalization {
    const char *name() const override { return "SimplifiedLayerNormalization"; }
};

// skip_layer_normalization (src/ops/norm/contrib.rs:22-77) on rten_hip_skip_norm_f32: sum = (input + skip) + bias, normalised over the last axis; `want_sum`
// also returns the sum (output 3, the residual stream), written by the same launch.  Outputs: [output] or [output, {}, {}, sum] -- the mean and
// inv_std_var slots (training outputs the reference fills with zeros) stay empty, the loader refuses a graph that reads them.
struct SkipNormBase : Operator {
    float epsilon = 1e-5f;
    bool want_sum = false;
    OutputList run_skip(Context &ctx, bool rms, const Tensor &x_in, const Tensor &skip_in, const Tensor &gamma, const Tensor *beta, const Tensor *bias) const {
        const Tensor &x = want(x_in, DType::F32, "float32"), &skip = want(skip_in, DType::F32, "float32");
        for (const Tensor *t : {&gamma, beta, bias}) {
            if (!t) continue;
            want(*t, DType::F32, "float32");
            if (t->ndim() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 1 dims");
        }
        if (x.ndim() != 2 && x.ndim() != 3) throw OpError(OpError::InvalidValue, "input must be 2 or 3 dimensioned");
        if (skip.ndim() != 2 && skip.ndim() != 3) throw OpError(OpError::InvalidValue, "skip must be 2 or 3 dimensioned");
        const bool tail = skip.size(skip.ndim() - 1) == x.size(x.ndim() - 1) && skip.size(skip.ndim() - 2) == x.size(x.ndim() - 2);
        if (!tail || skip.ndim() > x.ndim() || (skip.ndim() == 3 && skip.size(0) != 1 && skip.size(0) != x.size(0)))
            throw OpError(OpError::IncompatibleInputShapes, "skip must broadcast to input over the batch dimension");
        const int64_t cols = x.size(x.ndim() - 1), rows = cols ? x.len() / cols : 0;
        if (bias && bias->len() != 1 && bias->len() != cols) throw OpError(OpError::IncompatibleInputShapes, "Cannot broadcast inputs");
        float gs = 1.f, bs = 0.f;
        const bool one = decoder_detail::one_element(gamma, gs);
        if (!one && gamma.len() != cols) throw OpError(OpError::InvalidValue, "`scale` is not broadcastable to normalized axes of input");
        if (beta && beta->len() != 1 && beta->len() != cols) throw OpError(OpError::InvalidValue, "`bias` is not broadcastable to normalized axes of input");
        const bool beta_one = beta && decoder_detail::one_element(*beta, bs);
        OutputList out;
        out.emplace_back(ctx, x.shape(), DType::F32);
        if (want_sum) { out.emplace_back(); out.emplace_back(); }
        if (one || beta_one || (bias && bias->len() != cols)) {
            // a one-element gamma / beta is the reference's scalar form (other bits than a vector of equal values), a one-element bias a broadcast: the
            // operators one after the other, on the entry points that take a scalar
            OutputList sum = Add().run(ctx, {&x, &skip});
            if (bias) sum = Add().run(ctx, {&sum[0], bias});
            if (x.len()) {
                if (rms) ctx.check(rten_hip_rms_norm_f32(ctx.raw(), rows, (int32_t)cols, (const float *)sum[0].ptr(), one ? nullptr : (const float *)gamma.ptr(), gs, epsilon, (float *)out[0].ptr()));
                else ctx.check(rten_hip_layer_norm_f32(ctx.raw(), rows, (int32_t)cols, (const float *)sum[0].ptr(), one ? nullptr : (const float *)gamma.ptr(),
                                                       beta && !beta_one ? (const float *)beta->ptr() : nullptr, gs, bs, epsilon, (float *)out[0].ptr()));
            }
            if (want_sum) out.push_back(std::move(sum[0]));
            return out;
        }
        if (want_sum) out.emplace_back(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_skip_norm_f32(ctx.raw(), rms ? RTEN_HIP_SKIP_NORM_RMS : RTEN_HIP_SKIP_NORM_LAYER, rows, (int32_t)cols, (const float *)x.ptr(), (const float *)skip.ptr(),
                                             skip.len() / cols, (const float *)vp(bias), (const float *)gamma.ptr(), (const float *)vp(beta), epsilon,
                                             want_sum ? (float *)out[3].ptr() : nullptr, (float *)out[0].ptr()));
        return out;
    }
};
// SkipLayerNormalization (com.microsoft, src/ops/norm/contrib.rs:123-177): inputs input, skip, gamma, beta?, bias?; epsilon is a required attribute
struct SkipLayerNormalization : SkipNormBase {
    const char *name() const override { return "SkipLayerNormalization"; }
    int max_inputs() const override { return 5; }
    OutputList run(Context &ctx, const InputList &in) const override { return run_skip(ctx, false, require(in, 0), require(in, 1), require(in, 2), get(in, 3), get(in, 4)); }
};
// SkipSimplifiedLayerNormalization (com.microsoft, src/ops/norm/contrib.rs:186-238): the RMS form; inputs input, skip, gamma, bias?
struct SkipSimplifiedLayerNormalization : SkipNormBase {
    const char *name() const override { return "SkipSimplifiedLayerNormalisation"; } // (sic, contrib.rs:192)
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override { return run_skip(ctx, true, require(in, 0), require(in, 1), require(in, 2), nullptr, get(in, 3)); }
};

// Add(residual) -> RMSNormalization / SimplifiedLayerNormalization over the last axis as one skip launch (the executor's fusion): the sum is x + r, the
// one f32 add the Add node makes, so the result has the bits of the two operators.  `want_sum`: the sum has other readers (the residual stream) and is
// written by the same launch as a second output.  A one-element scale, or operands of different shapes, run the two operators one after the other.
struct AddRMSNormalization : Operator {
    float epsilon = 1e-5f;
    bool want_sum = false;
    const char *name() const override { return "AddRMSNormalization"; }
    int max_inputs() const override { return 3; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0), &r = require(in, 1), &scale = require(in, 2);
        const int64_t cols = x.ndim() ? x.size(x.ndim() - 1) : 1, rows = cols ? x.len() / cols : 0;
        OutputList out;
        if (x.dtype() != DType::F32 || r.dtype() != DType::F32 || scale.dtype() != DType::F32 || x.shape() != r.shape() || x.ndim() == 0 || scale.len() != cols || cols == 1) {
            OutputList sum = Add().run(ctx, {&x, &r});
            RMSNormalization norm;
            norm.epsilon = epsilon;
            out = norm.run(ctx, {&sum[0], &scale});
            if (want_sum) out.push_back(std::move(sum[0]));
            return out;
        }
        out.emplace_back(ctx, x.shape(), DType::F32);
        if (want_sum) out.emplace_back(ctx, x.shape(), DType::F32);
        if (x.len())
            ctx.check(rten_hip_skip_norm_f32(ctx.raw(), RTEN_HIP_SKIP_NORM_RMS, rows, (int32_t)cols, (const float *)x.ptr(), (const float *)r.ptr(), rows, nullptr,
                                             (const float *)scale.ptr(), nullptr, epsilon, want_sum ? (float *)out[1].ptr() : nullptr, (float *)out[0].ptr()));
        return out;
    }
};

// RotaryEmbedding (ai.onnx, src/ops/embedding.rs:209-252; loader defaults onnx_registry.rs:1832-1847): inputs X [B, S, H * D] (needs num_heads) or
// [B, H, S, D], cos, sin, position_ids [B, S]?
struct RotaryEmbedding : Operator {
    bool interleaved = false;
    int64_t num_heads = 0, rotary_embedding_dim = 0;
    const char *name() const override { return "RotaryEmbedding"; }
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor *ids = get(in, 3);
        if (ids && ids->ndim() != 2) throw OpError(OpError::InputCastFailed, "expected tensor with 2 dims");
        OutputList out;
        out.push_back(decoder_detail::rotary_embedding(ctx, require(in, 0), require(in, 1), require(in, 2), ids, false, interleaved, num_heads, rotary_embedding_dim));
        return out;
    }
};
// com.microsoft RotaryEmbedding (src/ops/embedding/contrib.rs:17-135): inputs X, position_ids, cos [max_pos, half], sin.  position_ids is [B, S], or a
// scalar / one-element vector holding an offset; num_heads 0 (the attribute's default, or absent) is inferred from the cache for a 3-D input.
struct RotaryEmbeddingMicrosoft : Operator {
    bool interleaved = false;
    int64_t num_heads = 0, rotary_embedding_dim = 0;
    const char *name() const override { return "com.microsoft.RotaryEmbedding"; }
    int max_inputs() const override { return 4; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &x = require(in, 0), &ids = require(in, 1), &cos = require(in, 2), &sin = require(in, 3);
        if (x.ndim() != 3 && x.ndim() != 4) throw OpError(OpError::IncompatibleInputShapes, "Input processed needs 3-4 dimensions");
        bool offset;
        if (ids.ndim() <= 1 && ids.len() == 1) offset = true;
        else if (ids.ndim() == 2) offset = false;
        else throw OpError(OpError::InvalidValue, "position_ids must be a scalar, a 1-element vector or have 2 dims");
        int64_t heads = num_heads;
        if (x.ndim() == 3 && heads == 0) {
            if (rotary_embedding_dim != 0) throw OpError(OpError::InvalidValue, "num_heads must be specified when rotary_embedding_dim is set");
            if (cos.ndim() == 0) throw OpError(OpError::InvalidValue, "cos cache must not be scalar");
            const int64_t half = cos.size(cos.ndim() - 1);
            if (half == 0) throw OpError(OpError::InvalidValue, "Last dimension of cos cache must not be 0");
            if (x.size(2) % (2 * half) != 0) throw OpError(OpError::InvalidValue, "hidden_size must be divisible by head size");
            heads = x.size(2) / (2 * half);
        }
        OutputList out;
        out.push_back(decoder_detail::rotary_embedding(ctx, x, cos, sin, &ids, offset, interleaved, heads, rotary_embedding_dim));
        return out;
    }
};

// GroupQueryAttention with a KV cache (com.microsoft, src/ops/attention/contrib.rs:419-878; loader defaults onnx_registry.rs:1467-1492) on rten_hip_gqa_f32:
// inputs query [B, S, H * D] (packed [B, S, (H + 2 KV) * D] with key and value absent), key, value [B, S, KV * D], past_key, past_value [B, KV, P, D],
// seqlens_k int32 [B] or [B, 1], total_sequence_length int32 scalar, cos_cache, sin_cache [max, rot / 2], position_ids int32 [B, S], attention_bias
// [B | 1, H | 1, >= S, >= P + S], head_sink (refused).  seqlens_k and total_sequence_length that carry a host copy (constants) are validated with the
// reference's errors (contrib.rs:582-639); values only the device knows stay there -- nothing is read back, the step captures -- and the kernels clamp
// kv_len into [1, P + S] and past_len into [0, P].  `want_present`: outputs 1 / 2 are requested (contrib.rs:803-807); the caches are computed either way,
// because the attention kernels read K and V out of them.
struct GroupQueryAttention : Operator {
    int64_t num_heads = 0, kv_num_heads = 0;
    std::optional<float> scale;
    bool do_rotary = false, rotary_interleaved = false, smooth_softmax = false, want_present = true;
    int64_t local_window_size = -1; // non-positive: no window
    float softcap = 0.f;
    const char *name() const override { return "com.microsoft.GroupQueryAttention"; }
    int max_inputs() const override { return 12; }
    OutputList run(Context &ctx, const InputList &in) const override {
        const Tensor &query = want(require(in, 0), DType::F32, "float32");
        if (query.ndim() != 3) throw OpError(OpError::InputCastFailed, "expected tensor with 3 dims");
        const Tensor *key = get(in, 1), *value = get(in, 2), *past_key = get(in, 3), *past_value = get(in, 4);
        const Tensor &seqlens = want(require(in, 5), DType::I32, "int32"), &total = want(require(in, 6), DType::I32, "int32");
        const Tensor *cos = get(in, 7), *sin = get(in, 8), *position_ids = get(in, 9), *bias = get(in, 10), *head_sink = get(in, 11);
        for (const Tensor *t : {key, value}) {
            if (!t) continue;
            want(*t, DType::F32, "float32");
            if (t->ndim() != 3) throw OpError(OpError::InputCastFailed, "expected tensor with 3 dims");
        }
        std::vector<int64_t> sl = seqlens.shape();
        while (sl.size() > 1 && sl.back() == 1) sl.pop_back();
        if (sl.size() != 1) throw OpError(OpError::UnsupportedValue, "seqlens_k must be a vector");
        if (total.len() != 1) throw OpError(OpError::InputCastFailed, "expected tensor with 0 dims");
        if (head_sink) throw OpError(OpError::UnsupportedValue, "head_sink is not supported");
        if (smooth_softmax) throw OpError(OpError::UnsupportedValue, "smooth_softmax is not supported");
        const int64_t H = num_heads, KV = kv_num_heads;
        if (H <= 0 || KV <= 0) throw OpError(OpError::InvalidValue, "num_heads and kv_num_heads must be positive");
        if (H % KV != 0) throw OpError(OpError::InvalidValue, "num_heads must be a multiple of kv_num_heads");
        const int64_t batch = query.size(0), seq = query.size(1), q_hidden = query.size(2);
        int64_t D, st[RTEN_HIP_GQA_NSTRIDES] = {};
        const float *qp = (const float *)query.ptr(), *kp, *vp_;
        if (key && value) {
            if (q_hidden % H != 0) throw OpError(OpError::IncompatibleInputShapes, "query hidden size must be divisible by num_heads");
            D = q_hidden / H;
            if (key->size(0) != batch || value->size(0) != batch) throw OpError(OpError::IncompatibleInputShapes, "key and value batch size must match query");
            if (key->size(1) != value->size(1) || key->size(2) != value->size(2)) throw OpError(OpError::IncompatibleInputShapes, "key and value must have the same shape");
            if (key->size(2) != KV * D) throw OpError(OpError::IncompatibleInputShapes, "key hidden size must equal kv_num_heads * head_size");
            if (key->size(1) != seq) throw OpError(OpError::UnsupportedValue, "key sequence length must match query sequence length");
            kp = (const float *)key->ptr(); vp_ = (const float *)value->ptr();
            st[0] = seq * H * D; st[1] = H * D; st[2] = D;
            st[3] = st[6] = seq * KV * D; st[4] = st[7] = KV * D; st[5] = st[8] = D;
        } else if (!key && !value) {
            const int64_t heads = H + 2 * KV;
            if (q_hidden % heads != 0) throw OpError(OpError::IncompatibleInputShapes, "packed query hidden size must be divisible by num_heads + 2 * kv_num_heads");
            D = q_hidden / heads;
            kp = qp + H * D; vp_ = qp + (H + KV) * D;
            for (int i = 0; i < 3; i++) { st[3 * i] = seq * q_hidden; st[3 * i + 1] = q_hidden; st[3 * i + 2] = D; }
        } else throw OpError(OpError::InvalidValue, "key and value must both be present or both absent");
        if (sl[0] != batch) throw OpError(OpError::IncompatibleInputShapes, "seqlens_k must have batch_size elements");
        const HostVal *total_h = total.host(), *seqlens_h = seqlens.host();
        if (total_h && total_h->is_float) total_h = nullptr;
        if (seqlens_h && seqlens_h->is_float) seqlens_h = nullptr;
        if (total_h && total_h->i.size() == 1 && total_h->i[0] <= 0) throw OpError(OpError::InvalidValue, "total_sequence_length must be positive");
        int64_t P = 0;
        if (past_key && past_value) {
            want(*past_key, DType::F32, "float32"); want(*past_value, DType::F32, "float32");
            if (past_key->ndim() != 4 || past_value->ndim() != 4) throw OpError(OpError::InputCastFailed, "expected tensor with 4 dims");
            if (past_key->shape() != past_value->shape() || past_key->size(0) != batch || past_key->size(1) != KV || past_key->size(3) != D)
                throw OpError(OpError::IncompatibleInputShapes, "past_key/past_value shape does not match");
            P = past_key->size(2);
        } else if (past_key || past_value) throw OpError(OpError::InvalidValue, "past_key and past_value must both be present or both absent");
        const int64_t present_seq = P + seq;
        if (total_h && total_h->i.size() == 1) {
            const int64_t tot = total_h->i[0];
            const bool first = seq == tot, subsequent = seq > 1 && seq != tot;
            if (subsequent && batch != 1) throw OpError(OpError::UnsupportedValue, "batch size must be 1 when sequence_length > 1 and a past context is given");
            if (!first && !subsequent && seq != 1) throw OpError(OpError::InvalidValue, "sequence_length must be 1 when query is not a prompt");
        }
        if (seqlens_h)
            for (int64_t v : seqlens_h->i) {
                if (v < 0 || v >= present_seq) throw OpError(OpError::InvalidValue, "seqlens_k entry is out of range");
                if (v + 1 < seq) throw OpError(OpError::InvalidValue, "seqlens_k entry is too small for the query sequence length");
            }
        if (bias) {
            want(*bias, DType::F32, "float32");
            if (bias->ndim() != 4) throw OpError(OpError::InputCastFailed, "expected tensor with 4 dims");
            const int64_t bb = bias->size(0), bh = bias->size(1), bs = bias->size(2), bt = bias->size(3);
            if ((bb != 1 && bb != batch) || (bh != 1 && bh != H) || bs < seq || bt < present_seq)
                throw OpError(OpError::IncompatibleInputShapes, "attention_bias shape is incompatible with query/key shapes");
            st[9] = bb == 1 ? 0 : bh * bs * bt; st[10] = bh == 1 ? 0 : bs * bt; st[11] = bt;
        }
        const float sc = scale ? *scale : (D ? 1.0f / std::sqrt((float)D) : 0.f);
        int64_t rot = 0, max_pos = 0;
        if (do_rotary) {
            if (!cos || !sin) throw OpError(OpError::InvalidValue, "cos_cache and sin_cache are required when do_rotary is set");
            want(*cos, DType::F32, "float32"); want(*sin, DType::F32, "float32");
            if (cos->ndim() != 2 || sin->ndim() != 2) throw OpError(OpError::InputCastFailed, "expected tensor with 2 dims");
            rot = 2 * cos->size(1);
            if (rot == 0) throw OpError(OpError::InvalidValue, "rotary_embedding_dim must be a positive even number");
            if (rot > D) throw OpError(OpError::InvalidValue, "rotary_embedding_dim must not exceed head size");
            if (sin->size(1) != cos->size(1)) throw OpError(OpError::InvalidValue, "Last dimension of sin cache does not match rotary_embedding_dim/2");
            if (cos->size(0) != sin->size(0)) throw OpError(OpError::UnsupportedValue, "device path needs cos and sin caches of one length");
            max_pos = cos->size(0);
            if (position_ids) {
                want(*position_ids, DType::I32, "int32");
                if (position_ids->ndim() != 2) throw OpError(OpError::InputCastFailed, "expected tensor with 2 dims");
                if (position_ids->size(0) != batch || position_ids->size(1) != seq)
                    throw OpError(OpError::UnsupportedValue, "device path needs position_ids of the input's [batch, seq] shape");
                if (const HostVal *h = position_ids->host())
                    if (!h->is_float)
                        for (int64_t v : h->i)
                            if (v < -max_pos || v >= max_pos) throw OpError(OpError::InvalidValue, "Entry in `indices` is out of range");
            }
        }
        if (softcap != 0.f) throw OpError(OpError::UnsupportedValue, "softcap is not supported");
        OutputList out;
        out.emplace_back(ctx, std::vector<int64_t>{batch, seq, H * D}, DType::F32);
        out.emplace_back(ctx, std::vector<int64_t>{batch, KV, present_seq, D}, DType::F32);
        out.emplace_back(ctx, std::vector<int64_t>{batch, KV, present_seq, D}, DType::F32);
        if (out[0].len() && out[1].len()) {
            const int32_t dims[RTEN_HIP_GQA_NDIMS] = {(int32_t)batch, (int32_t)seq, (int32_t)H, (int32_t)KV, (int32_t)D, (int32_t)P, (int32_t)rot, rotary_interleaved ? 1 : 0,
                                                      (int32_t)max_pos, (int32_t)(local_window_size > 0 ? local_window_size : 0)};
            ctx.check(rten_hip_gqa_f32(ctx.raw(), dims, st, sc, qp, kp, vp_, (const float *)vp(past_key), (const float *)vp(past_value), (const int32_t *)seqlens.ptr(),
                                       (const int32_t *)total.ptr(), do_rotary ? (const float *)cos->ptr() : nullptr, do_rotary ? (const float *)sin->ptr() : nullptr,
                                       do_rotary ? (const int32_t *)vp(position_ids) : nullptr, (const float *)vp(bias), (float *)out[0].ptr(), (float *)out[1].ptr(),
                                       (float *)out[2].ptr()));
        }
        if (!want_present) out.resize(1);
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ registry (src/op_registry.rs:25-72)
class OpRegistry {
  public:
    using Factory = std::function<std::unique_ptr<Operator>()>;
    template <typename Op> void register_op(const std::string &name) { factories_[name] = [] { return std::unique_ptr<Operator>(new Op()); }; }
    std::unique_ptr<Operator> create(const std::string &name) const {
        auto it = factories_.find(name);
        if (it == factories_.end()) throw OpError(OpError::UnsupportedValue, "operator not registered: " + name); // ReadOpError::OperatorUnavailable
        return it->second();
    }
    bool contains(const std::string &name) const { return factories_.count(name) != 0; }
    std::vector<std::string> names() const {
        std::vector<std::string> v;
        for (auto &kv : factories_) v.push_back(kv.first);
        return v;
    }
    static OpRegistry with_all_ops() { // every hot-path operator this backend overrides
        OpRegistry r;
        r.register_op<Conv>("Conv");
        r.register_op<ConvTranspose>("ConvTranspose");
        r.register_op<ConvInteger>("ConvInteger");
        r.register_op<ConvIntegerToFloat>("ConvIntegerToFloat");
        r.register_op<MatMul>("MatMul");
        r.register_op<FusedMatMul>("FusedMatMul");
        r.register_op<Gemm>("Gemm");
        r.register_op<MatMulInteger>("MatMulInteger");
        r.register_op<MatMulNBits>("MatMulNBits");
        r.register_op<Softmax>("Softmax");
        r.register_op<LogSoftmax>("LogSoftmax");
        r.register_op<LayerNormalization>("LayerNormalization");
        r.register_op<BatchNormalization>("BatchNormalization");
        r.register_op<InstanceNormalization>("InstanceNormalization");
        r.register_op<Relu>("Relu");
        r.register_op<Gelu>("Gelu");
        r.register_op<Erf>("Erf");
        r.register_op<Sigmoid>("Sigmoid");
        r.register_op<Silu>("Silu");
        r.register_op<Swish>("Swish");
        r.register_op<HardSigmoid>("HardSigmoid");
        r.register_op<HardSwish>("HardSwish");
        r.register_op<Clip>("Clip");
        r.register_op<LeakyRelu>("LeakyRelu");
        r.register_op<Elu>("Elu");
        r.register_op<Add>("Add");
        r.register_op<Mul>("Mul");
        r.register_op<Sub>("Sub");
        r.register_op<Div>("Div");
        r.register_op<Transpose>("Transpose");
        r.register_op<Gather>("Gather");
        r.register_op<AddSoftmax>("AddSoftmax");
        r.register_op<MaxPool>("MaxPool");
        r.register_op<AveragePool>("AveragePool");
        r.register_op<GlobalAveragePool>("GlobalAveragePool");
        r.register_op<DynamicQuantizeLinear>("DynamicQuantizeLinear");
        r.register_op<Cast>("Cast");
        r.register_op<Tanh>("Tanh");
        r.register_op<Where>("Where");
        r.register_op<ReduceSum>("ReduceSum");
        r.register_op<ReduceMean>("ReduceMean");
        r.register_op<Einsum>("Einsum");
        r.register_op<Resize>("Resize");
        r.register_op<Upsample>("Upsample");
        r.register_op<Split>("Split");
        r.register_op<ReduceMax>("ReduceMax");
        r.register_op<ReduceMin>("ReduceMin");
        r.register_op<ArgMax>("ArgMax");
        r.register_op<ArgMin>("ArgMin");
        r.register_op<TopK>("TopK");
        r.register_op<GRU>("GRU");
        r.register_op<LSTM>("LSTM");
        r.register_op<Neg>("Neg");
        r.register_op<Abs>("Abs");
        r.register_op<Sign>("Sign");
        r.register_op<Floor>("Floor");
        r.register_op<Ceil>("Ceil");
        r.register_op<Round>("Round");
        r.register_op<Sqrt>("Sqrt");
        r.register_op<Reciprocal>("Reciprocal");
        r.register_op<Exp>("Exp");
        r.register_op<Log>("Log");
        r.register_op<Softplus>("Softplus");
        r.register_op<Pow>("Pow");
        r.register_op<PRelu>("PRelu");
        r.register_op<Min>("Min");
        r.register_op<Max>("Max");
        r.register_op<Sum>("Sum");
        r.register_op<Mean>("Mean");
        r.register_op<Pad>("Pad");
        r.register_op<QuantizeLinear>("QuantizeLinear");
        r.register_op<DequantizeLinear>("DequantizeLinear");
        r.register_op<ReduceL1>("ReduceL1");
        r.register_op<ReduceL2>("ReduceL2");
        r.register_op<ReduceSumSquare>("ReduceSumSquare");
        r.register_op<ReduceLogSum>("ReduceLogSum");
        r.register_op<ReduceLogSumExp>("ReduceLogSumExp");
        r.register_op<ReduceProd>("ReduceProd");
        r.register_op<LpNormalization>("LpNormalization");
        r.register_op<GlobalMaxPool>("GlobalMaxPool");
        r.register_op<GridSample>("GridSample");
        r.register_op<DepthToSpace>("DepthToSpace");
        r.register_op<CumSum>("CumSum");
        r.register_op<NonMaxSuppression>("NonMaxSuppression");
        r.register_op<DFT>("DFT");
        r.register_op<STFT>("STFT");
        r.register_op<GatherElements>("GatherElements");
        r.register_op<Trilu>("Trilu");
        r.register_op<Tile>("Tile");
        r.register_op<RMSNormalization>("RMSNormalization");
        r.register_op<SimplifiedLayerNormalization>("SimplifiedLayerNormalization"); // ai.onnx (sic, onnx_registry.rs:275)
        r.register_op<RotaryEmbedding>("RotaryEmbedding");
        // the contrib operators (onnx_registry.rs:285-296) under their domain: the loader dispatches on it, as the reference's OpId does
        r.register_op<SkipLayerNormalization>("com.microsoft.SkipLayerNormalization");
        r.register_op<SkipSimplifiedLayerNormalization>("com.microsoft.SkipSimplifiedLayerNormalization");
        r.register_op<RotaryEmbeddingMicrosoft>("com.microsoft.RotaryEmbedding");
        r.register_op<GroupQueryAttention>("com.microsoft.GroupQueryAttention");
        return r;
    }

  private:
    std::map<std::string, Factory> factories_;
};

} // namespace rten_hip
