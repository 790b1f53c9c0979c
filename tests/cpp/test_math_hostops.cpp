// Host evaluation of the math operators and of constant-mode Pad (include/rten_hip_graph.hpp, namespace hostops): the values exporter-written graphs compute
// from input shapes (F.interpolate(scale_factor=..) as Shape -> Cast -> Mul -> Floor -> Cast, attention scaling as Sqrt(Cast(Shape[-1])), padded shape
// vectors).  The semantics are the device's (tests/math_rules.py): Rust signum, ties to even, NaN and tie placement of Min / Max.  Needs no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "rten_hip_graph.hpp"

using namespace rten_hip;
static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static HostVal ints(std::vector<int64_t> shape, std::vector<int64_t> v) { return hostops::make_ints(std::move(shape), std::move(v)); }
static HostVal floats(std::vector<int64_t> shape, std::vector<float> v) { HostVal h; h.shape = std::move(shape); h.is_float = true; h.f = std::move(v); return h; }
static uint32_t bits(float v) { uint32_t w; std::memcpy(&w, &v, 4); return w; }
// bitwise equality, any NaN equal to any NaN
static bool same(const std::vector<float> &a, const std::vector<float> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (!(bits(a[i]) == bits(b[i]) || (a[i] != a[i] && b[i] != b[i]))) { std::printf("  element %zu: %.9g (%08x) vs %.9g (%08x)\n", i, a[i], bits(a[i]), b[i], bits(b[i])); return false; }
    return true;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int64_t imin = std::numeric_limits<int32_t>::min(), imax = std::numeric_limits<int32_t>::max();
    HostVal out;
    // ---- unary, float32
    const HostVal x = floats({8}, {0.f, -0.f, 2.5f, -0.4f, nan, inf, -inf, -3.5f});
    CHECK(hostops::unary("Sign", x, out) && out.is_float && same(out.f, {1.f, -1.f, 1.f, -1.f, nan, 1.f, -1.f, -1.f}));  // Rust signum, not ONNX's 0
    CHECK(hostops::unary("Round", x, out) && same(out.f, {0.f, -0.f, 2.f, -0.f, nan, inf, -inf, -4.f}));                 // ties to even; -0.4 -> -0.0
    CHECK(hostops::unary("Round", floats({4}, {0.5f, 1.5f, 3.5f, -2.5f}), out) && same(out.f, {0.f, 2.f, 4.f, -2.f}));
    CHECK(hostops::unary("Floor", x, out) && same(out.f, {0.f, -0.f, 2.f, -1.f, nan, inf, -inf, -4.f}));
    CHECK(hostops::unary("Ceil", x, out) && same(out.f, {0.f, -0.f, 3.f, -0.f, nan, inf, -inf, -3.f}));
    CHECK(hostops::unary("Neg", x, out) && same(out.f, {-0.f, 0.f, -2.5f, 0.4f, nan, -inf, inf, 3.5f}));
    CHECK(hostops::unary("Abs", x, out) && same(out.f, {0.f, 0.f, 2.5f, 0.4f, nan, inf, inf, 3.5f}));
    CHECK(hostops::unary("Sqrt", floats({6}, {64.f, 2.f, 0.f, -0.f, -1.f, inf}), out) && same(out.f, {8.f, 1.41421354f, 0.f, -0.f, nan, inf}));
    CHECK(hostops::unary("Reciprocal", floats({5}, {2.f, 0.f, -0.f, 3.f, inf}), out) && same(out.f, {0.5f, inf, -inf, 0.333333343f, 0.f}));
    CHECK(out.shape == std::vector<int64_t>{5});
    // ---- unary, int32: wrapping
    const HostVal xi = ints({5}, {imin, imax, -7, 0, 5});
    CHECK(hostops::unary("Neg", xi, out) && !out.is_float && out.i == std::vector<int64_t>({imin, -imax, 7, 0, -5}));
    CHECK(hostops::unary("Abs", xi, out) && out.i == std::vector<int64_t>({imin, imax, 7, 0, 5}));
    CHECK(hostops::unary("Sign", xi, out) && out.i == std::vector<int64_t>({-1, 1, -1, 0, 1}));
    CHECK(!hostops::unary("Floor", xi, out) && !hostops::unary("Sqrt", xi, out)); // float32 only: declined, the device path reports the type error
    CHECK(!hostops::unary("Exp", x, out) && !hostops::unary("Log", x, out));      // never on the host
    // ---- Min / Max: a NaN in either operand wins, a tie keeps the left operand
    CHECK(hostops::minmax(false, floats({1}, {0.f}), floats({1}, {-0.f}), out) && bits(out.f[0]) == bits(0.f));
    CHECK(hostops::minmax(false, floats({1}, {-0.f}), floats({1}, {0.f}), out) && bits(out.f[0]) == bits(-0.f));
    CHECK(hostops::minmax(true, floats({1}, {0.f}), floats({1}, {-0.f}), out) && bits(out.f[0]) == bits(0.f));
    CHECK(hostops::minmax(true, floats({1}, {-0.f}), floats({1}, {0.f}), out) && bits(out.f[0]) == bits(-0.f));
    CHECK(hostops::minmax(false, floats({3}, {1.f, nan, 3.f}), floats({3}, {nan, 1.f, 2.f}), out) && same(out.f, {nan, nan, 3.f}));
    CHECK(hostops::minmax(true, floats({3}, {1.f, nan, 3.f}), floats({3}, {nan, 1.f, 2.f}), out) && same(out.f, {nan, nan, 2.f}));
    CHECK(hostops::minmax(true, ints({2, 1}, {imin, 4}), ints({3}, {3, imax, -1}), out) && out.shape == (std::vector<int64_t>{2, 3}) && out.i == std::vector<int64_t>({imin, imin, imin, 3, 4, -1}));
    CHECK(!hostops::minmax(true, ints({1}, {1}), floats({1}, {1.f}), out)); // mixed types: declined
    // variadic: a left fold with broadcasting; one operand is a copy
    const HostVal a = ints({2}, {2, 4}), b = ints({}, {3}), c = ints({2, 2}, {1, 2, 3, 4});
    CHECK(hostops::minmax_fold(false, {&a, &b, &c}, out) && out.shape == (std::vector<int64_t>{2, 2}) && out.i == std::vector<int64_t>({3, 4, 3, 4})); // variadic_elementwise.rs:272-279
    CHECK(hostops::minmax_fold(true, {&a}, out) && out.shape == a.shape && out.i == a.i);
    CHECK(!hostops::minmax_fold(true, {}, out));
    // the dynamic-upsample idiom: Floor(Cast(Shape) * 2.0) -> Cast
    HostVal scaled, fl;
    CHECK(hostops::binary("Mul", hostops::cast(ints({2}, {7, 9}), DType::F32), floats({}, {1.5f}), scaled) && hostops::unary("Floor", scaled, fl) && same(fl.f, {10.f, 13.f}));
    CHECK(hostops::cast(fl, DType::I32).i == std::vector<int64_t>({10, 13}));
    // ---- constant Pad of a host value
    const HostVal v = ints({5}, {1, 2, 3, 4, 5});
    CHECK(hostops::pad_constant(v, {-2, 1}, nullptr, out) && out.shape == std::vector<int64_t>{4} && out.i == std::vector<int64_t>({3, 4, 5, 0}));   // pad.rs:451-456
    CHECK(hostops::pad_constant(v, {-1, -2}, nullptr, out) && out.shape == std::vector<int64_t>{2} && out.i == std::vector<int64_t>({2, 3}));      // pad.rs:444-449
    const HostVal seven = ints({}, {7});
    CHECK(hostops::pad_constant(v, {2, -3}, &seven, out) && out.i == std::vector<int64_t>({7, 7, 1, 2}));
    CHECK(hostops::pad_constant(ints({3}, {1, 2, 3}), {-1, -2}, nullptr, out) && out.shape == std::vector<int64_t>{0} && out.i.empty());            // pad.rs:458-463
    const HostVal m2 = floats({2, 3}, {1.f, 2.f, 3.f, 4.f, 5.f, 6.f}), fillf = floats({}, {-0.5f});
    CHECK(hostops::pad_constant(m2, {1, -1, 0, 1}, &fillf, out) && out.shape == (std::vector<int64_t>{3, 3}) &&
          same(out.f, {-0.5f, -0.5f, -0.5f, 2.f, 3.f, -0.5f, 5.f, 6.f, -0.5f}));
    CHECK(!hostops::pad_constant(m2, {0, 0, 0, 0}, &seven, out)); // a fill of another type: declined, the device path reports it
    auto refused = [&](const HostVal &t, std::vector<int64_t> pads, const char *msg) {
        try { hostops::pad_constant(t, pads, nullptr, out); } catch (const OpError &e) { return std::string(e.what()).find(msg) != std::string::npos; }
        return false;
    };
    CHECK(refused(m2, {1}, "padding length should be 2 * input dims"));
    CHECK(refused(m2, {-3, 0, 0, 0}, "Negative pads remove more elements than axis contains"));
    // the shape checks shared with the device operator
    bool threw = false;
    try { pad_geometry({1, 1, 3}, {0, 0, 0, 2, 0, 0}, RTEN_HIP_PAD_REFLECT); } catch (const OpError &e) { threw = std::string(e.what()).find("Pad only supports non-constant padding of last 2 dims") != std::string::npos; }
    CHECK(threw);
    threw = false;
    try { pad_geometry({3, 0}, {0, 2, 0, 0}, RTEN_HIP_PAD_EDGE); } catch (const OpError &e) { threw = std::string(e.what()).find("Padded dimension for non-constant padding is empty") != std::string::npos; }
    CHECK(threw);
    CHECK(pad_geometry({1, 3}, {0, -1, 0, -2}, RTEN_HIP_PAD_REFLECT).copy);                                  // an emptied axis without padding: the empty crop (pad.rs:584-589)
    CHECK(pad_geometry({2, 3, 4, 5}, {-1, 0, 1, 2, 0, 0, 3, 4}, RTEN_HIP_PAD_WRAP).out == (std::vector<int64_t>{1, 3, 8, 11})); // a CROP of a batch dim is allowed
    CHECK(pad_mode_of("reflect") == RTEN_HIP_PAD_REFLECT && pad_mode_of("mirror") < 0);
    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
