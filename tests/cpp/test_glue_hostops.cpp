// Host evaluation of the glue operators (include/rten_hip_graph.hpp, namespace hostops) over the table of tests/glue_cases.py: reads the cases
// tests/test_glue_ops.py writes, evaluates each the way Graph::make_layout_step does when every operand carries a host value, and writes the
// result -- values as raw words, an OpError as kind and message, or DECLINED when the host path hands the node to the device.  Needs no GPU.
//
//   test_glue_hostops <cases file> <results file>
//
// cases:    CASE <id> <op> / ATTR <name> <n> <ints...> / VALUE f <hex word> | VALUE i <int64> / IN f|i <rank> <dims...> <n> <hex words...> / END
// results:  CASE <id> / OK f|i <rank> <dims...> <n> <hex words...> | ERR <kind> <message> | DECLINED
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>

#include "rten_hip_graph.hpp"

using namespace rten_hip;

struct Case {
    std::string id, op;
    std::map<std::string, std::vector<int64_t>> attrs;
    bool has_value = false;
    HostVal value;
    std::vector<HostVal> in;
};

static HostVal read_tensor(std::istream &s) {
    std::string ty;
    size_t rank, n;
    HostVal h;
    s >> ty >> rank;
    h.is_float = ty == "f";
    h.shape.resize(rank);
    for (auto &d : h.shape) s >> d;
    s >> n;
    for (size_t k = 0; k < n; k++) {
        std::string w;
        s >> w;
        const uint32_t bits = (uint32_t)std::stoul(w, nullptr, 16);
        if (h.is_float) { float f; std::memcpy(&f, &bits, 4); h.f.push_back(f); }
        else h.i.push_back((int64_t)(int32_t)bits);
    }
    return h;
}

static void write_tensor(std::ostream &o, const HostVal &h) {
    o << "OK " << (h.is_float ? "f " : "i ") << h.shape.size();
    for (int64_t d : h.shape) o << " " << d;
    const size_t n = h.is_float ? h.f.size() : h.i.size();
    o << " " << n << std::hex;
    for (size_t k = 0; k < n; k++) {
        uint32_t bits;
        if (h.is_float) std::memcpy(&bits, &h.f[k], 4); else bits = (uint32_t)(int32_t)h.i[k];
        o << " " << bits;
    }
    o << std::dec << "\n";
}

static int64_t attr1(const Case &c, const char *name, int64_t dflt) {
    auto it = c.attrs.find(name);
    return it == c.attrs.end() || it->second.empty() ? dflt : it->second[0];
}

// false: the host path declines (the device operator runs the node)
static bool evaluate(const Case &c, HostVal &out) {
    const std::string &op = c.op;
    std::vector<const HostVal *> v;
    for (auto &t : c.in) v.push_back(&t);
    if (op == "Shape") { out = hostops::shape_of(c.in.at(0).shape, attr1(c, "start", 0), c.attrs.count("end") != 0, attr1(c, "end", 0)); return true; }
    if (op == "Add" || op == "Sub" || op == "Mul" || op == "Div" || op == "And" || op == "Or" || op == "Xor" || op == "Equal" || op == "Less" || op == "LessOrEqual" ||
        op == "Greater" || op == "GreaterOrEqual")
        return hostops::binary(op, c.in.at(0), c.in.at(1), out);
    if (op == "Not") return hostops::logical_not(c.in.at(0), out);
    if (op == "Where") return hostops::where(c.in.at(0), c.in.at(1), c.in.at(2), out);
    if (op == "Cast") {
        const int64_t to = attr1(c, "to", onnx::FLOAT);
        if (to != onnx::FLOAT && to != onnx::INT32 && to != onnx::INT64) return false; // 8-bit results have no host value
        out = hostops::cast(c.in.at(0), to == onnx::FLOAT ? DType::F32 : DType::I32);
        return true;
    }
    if (op == "Transpose") {
        std::vector<int> perm;
        if (c.attrs.count("perm")) for (int64_t p : c.attrs.at("perm")) perm.push_back((int)p);
        out = hostops::transpose(c.in.at(0), perm);
        return true;
    }
    if (op == "Gather") { if (c.in.at(1).is_float) return false; out = hostops::gather(c.in.at(0), c.in.at(1), (int)attr1(c, "axis", 0)); return true; }
    if (op == "Concat") { out = hostops::concat(v, (int)attr1(c, "axis", 0)); return true; }
    if (op == "Slice") {
        const bool attr_form = c.attrs.count("starts") != 0;
        auto ints = [&](size_t k) { return c.in.size() > k ? c.in[k].i : std::vector<int64_t>(); };
        auto at = [&](const char *n) { return c.attrs.count(n) ? c.attrs.at(n) : std::vector<int64_t>(); };
        const std::vector<SliceRange> r = attr_form ? resolve_slice(c.in.at(0).shape, at("starts"), at("ends"), at("axes"), {})
                                                    : resolve_slice(c.in.at(0).shape, ints(1), ints(2), ints(3), ints(4));
        out = hostops::slice(c.in.at(0), r);
        return true;
    }
    if (op == "Expand") { out = hostops::expand(c.in.at(0), c.in.at(1).i); return true; }
    if (op == "ConstantOfShape") {
        HostVal fill;
        fill.is_float = true; fill.f = {0.f};
        if (c.has_value) fill = c.value;
        out = hostops::constant_fill(fill, c.in.at(0).i);
        return true;
    }
    if (op == "Flatten" || op == "Reshape" || op == "Squeeze" || op == "Unsqueeze") { // the views: a shape computed on the host, the same values under it
        const bool have_spec = c.in.size() > 1;
        out = hostops::reshaped(c.in.at(0), hostops::view_shape(op, c.in.at(0).shape, have_spec ? c.in[1].i : std::vector<int64_t>(), have_spec, (int)attr1(c, "axis", 1),
                                                               attr1(c, "allowzero", 0) != 0));
        return true;
    }
    if (op == "NonZero") { out = hostops::nonzero(c.in.at(0)); return true; }
    if (op == "Range") { out = hostops::range(c.in.at(0), c.in.at(1), c.in.at(2)); return true; }
    throw std::runtime_error("test_glue_hostops: no host evaluation for " + op);
}

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: test_glue_hostops <cases> <results>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::ofstream res(argv[2]);
    if (!in || !res) { std::fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]); return 2; }
    std::string tok;
    Case c;
    size_t count = 0;
    while (in >> tok) {
        if (tok == "CASE") { c = Case(); in >> c.id >> c.op; }
        else if (tok == "ATTR") { std::string name; size_t n; in >> name >> n; auto &a = c.attrs[name]; a.resize(n); for (auto &x : a) in >> x; }
        else if (tok == "VALUE") {
            std::string ty, w;
            in >> ty >> w;
            c.has_value = true;
            c.value = HostVal();
            if (ty == "f") { const uint32_t bits = (uint32_t)std::stoul(w, nullptr, 16); float f; std::memcpy(&f, &bits, 4); c.value.is_float = true; c.value.f = {f}; }
            else c.value.i = {hostops::saturate32(std::stoll(w))}; // the int64 payload of the attribute, narrowed as Graph::make_layout_step narrows it
        }
        else if (tok == "IN") c.in.push_back(read_tensor(in));
        else if (tok == "END") {
            res << "CASE " << c.id << "\n";
            try {
                HostVal out;
                if (evaluate(c, out)) write_tensor(res, out); else res << "DECLINED\n";
            } catch (const OpError &e) {
                res << "ERR " << OpError::kind_name(e.kind) << " " << e.msg << "\n";
            }
            count++;
        } else { std::fprintf(stderr, "unexpected token %s\n", tok.c_str()); return 2; }
    }
    res.close();
    std::printf("evaluated %zu cases\n", count);
    return 0;
}
