// graph_session model.onnx script.txt          (graph_session --check-script script.txt: parse only, needs no device)
//
// One Context with the buffer pool on (as rten_hip_run has it), ONE Graph, and a script of actions on it: the way the executor is meant to be used --
// loaded once, then run at changing input shapes, captured, replayed, re-captured and re-planned.  One action per line, words separated by blanks,
// `#` starts a comment; IN / OUT / FILE are paths (Safetensors, except the plan tables), TAG is any word:
//   run IN OUT         an eager run on fresh feed tensors; the outputs are read back and released before the next action
//   hold IN TAG        an eager run whose outputs stay on the device under TAG while later actions run
//   read TAG OUT       first takes and fills pool buffers of every held output's byte size (the scribble of graph_outputs_outlive_run.cpp), then reads TAG's outputs
//   distinct TAG TAG   fails if an output tensor of one held run has the device address of an output of the other (compares addresses, reads nothing)
//   capture IN OUT     Graph::capture on feed tensors that stay, one replay, the captured outputs
//   refill IN          new values of the SAME shapes into the captured feed tensors
//   replay OUT         Graph::replay, the captured outputs
//   tune IN            Graph::autotune, reps 1
//   shape-plans FILE   Graph::set_shape_plans    } FILE: one entry per line, `KEY variant mode groups order` (KEY: "gemm:MxKxN" / a step name)
//   plan FILE          Graph::apply_plan         }
// Inputs are F32, or integers (I64 narrowed to int32 as the loader narrows the model's).  Every step of the plan is printed as `step KIND:NAME` first.
// Exit codes and error text follow graph_outputs_outlive_run; an error of an action names the script's line.
#include "rten_hip_graph.hpp"
#include "rten_hip_safetensors.hpp"

#include <sstream>

using namespace rten_hip;

struct Action { size_t line; std::vector<std::string> w; };

static std::vector<Action> parse_script(const std::string &path) {
    static const std::map<std::string, size_t> arity = {{"run", 2}, {"hold", 2}, {"read", 2}, {"distinct", 2}, {"capture", 2}, {"refill", 1}, {"replay", 1},
                                                        {"tune", 1}, {"shape-plans", 1}, {"plan", 1}};
    std::ifstream f(path);
    if (!f) throw GraphError("cannot open script " + path);
    std::vector<Action> acts;
    std::string text;
    for (size_t line = 1; std::getline(f, text); line++) {
        std::istringstream ss(text.substr(0, text.find('#')));
        Action a{line, {}};
        for (std::string word; ss >> word;) a.w.push_back(word);
        if (a.w.empty()) continue;
        auto it = arity.find(a.w[0]);
        if (it == arity.end()) throw GraphError("line " + std::to_string(line) + ": unknown action " + a.w[0]);
        if (a.w.size() != it->second + 1) throw GraphError("line " + std::to_string(line) + ": " + a.w[0] + " takes " + std::to_string(it->second) + " operand(s)");
        acts.push_back(std::move(a));
    }
    return acts;
}

static std::map<std::string, GemmPlan> read_plan_table(const std::string &path) {
    std::ifstream f(path);
    if (!f) throw GraphError("cannot open plan table " + path);
    std::map<std::string, GemmPlan> t;
    std::string key;
    GemmPlan p;
    while (f >> key >> p.variant >> p.mode >> p.groups >> p.order) { p.set = true; t[key] = p; }
    if (!f.eof()) throw GraphError("plan table " + path + ": malformed entry after " + std::to_string(t.size()) + " entries");
    return t;
}

// the host bytes of one graph input as the device takes them
static std::string input_bytes(const onnx::ValueInfo &in, const safetensors::Entry &e, DType &dt) {
    const bool is_f32 = in.elem_type == onnx::FLOAT;
    dt = is_f32 ? DType::F32 : in.elem_type == onnx::UINT8 ? DType::U8 : in.elem_type == onnx::INT8 ? DType::I8 : DType::I32;
    if (e.shape.size() != in.dims.size()) throw GraphError("input " + in.name + ": the Safetensors tensor has a different rank");
    for (size_t i = 0; i < e.shape.size(); i++)
        if (in.dims[i] >= 0 && in.dims[i] != e.shape[i]) throw GraphError("input " + in.name + ": the Safetensors tensor does not match the model's fixed dimensions");
    if (e.dtype == "I64" && dt == DType::I32) {
        std::string out((size_t)e.len() * 4, '\0');
        for (int64_t i = 0; i < e.len(); i++) { int64_t v; std::memcpy(&v, e.data.data() + 8 * i, 8); const int32_t x = (int32_t)v; std::memcpy(&out[(size_t)(4 * i)], &x, 4); }
        return out;
    }
    const char *want = dt == DType::F32 ? "F32" : dt == DType::I32 ? "I32" : dt == DType::U8 ? "U8" : "I8";
    if (e.dtype != want) throw GraphError("input " + in.name + ": Safetensors dtype " + e.dtype + " does not fit the model input");
    return e.data;
}

struct FeedSet {
    std::vector<Tensor> store;
    Graph::Feeds feeds;
};

// fresh device tensors for every graph input, or -- `into` -- new values for existing ones of the same shapes
static void load_feeds(Context &ctx, const Graph &g, const std::string &path, FeedSet &fs, bool into) {
    const auto given = safetensors::read(path);
    if (!into) { fs.store.clear(); fs.feeds.clear(); fs.store.reserve(g.inputs().size()); }
    else if (fs.store.size() != g.inputs().size()) throw GraphError("refill: nothing is captured");
    for (size_t k = 0; k < g.inputs().size(); k++) {
        const onnx::ValueInfo &in = g.inputs()[k];
        auto it = given.find(in.name);
        if (it == given.end()) throw GraphError("input " + in.name + " is missing from " + path);
        DType dt;
        const std::string host = input_bytes(in, it->second, dt);
        if (into) {
            if (fs.store[k].shape() != it->second.shape) throw GraphError("refill: input " + in.name + " has another shape than the captured feed");
        } else {
            fs.store.emplace_back(ctx, it->second.shape, dt);
            fs.feeds.emplace_back(in.name, &fs.store.back());
        }
        if (host.size() != fs.store[k].bytes()) throw GraphError("input " + in.name + ": " + std::to_string(host.size()) + " bytes for a tensor of " + std::to_string(fs.store[k].bytes()));
        if (!host.empty()) ctx.check(rten_hip_memcpy_h2d(ctx.raw(), fs.store[k].ptr(), host.data(), host.size()));
    }
}

static void save_outputs(Context &ctx, const Graph &g, const std::vector<Tensor> &outs, const std::string &path) {
    std::vector<std::pair<std::string, safetensors::Entry>> all;
    for (size_t i = 0; i < outs.size(); i++) {
        safetensors::Entry e;
        e.dtype = outs[i].dtype() == DType::F32 ? "F32" : outs[i].dtype() == DType::I32 ? "I32" : outs[i].dtype() == DType::U8 ? "U8" : "I8";
        e.shape = outs[i].shape();
        e.data.resize(outs[i].bytes());
        if (outs[i].bytes()) ctx.check(rten_hip_memcpy_d2h(ctx.raw(), &e.data[0], outs[i].ptr(), outs[i].bytes()));
        all.emplace_back(g.outputs()[i].name, std::move(e));
    }
    safetensors::write(path, all);
}

int main(int argc, char **argv) {
    const bool check_only = argc == 3 && std::string(argv[1]) == "--check-script";
    if (argc != 3) { std::fprintf(stderr, "usage: graph_session model.onnx script.txt | graph_session --check-script script.txt\n"); return 1; }
    size_t line = 0;
    std::string what;
    try {
        const std::vector<Action> script = parse_script(argv[2]);
        if (check_only) { // the host-only half: the script, and every input and plan file it names that exists, read and (Safetensors) written back to memory
            size_t files = 0;
            for (auto &a : script) {
                line = a.line; what = a.w[0];
                if (a.w[0] == "shape-plans" || a.w[0] == "plan") { std::printf("line %zu: %s, %zu entries\n", a.line, a.w[0].c_str(), read_plan_table(a.w[1]).size()); files++; }
                else if (a.w[0] == "run" || a.w[0] == "hold" || a.w[0] == "capture" || a.w[0] == "refill" || a.w[0] == "tune") {
                    const auto t = safetensors::read(a.w[1]);
                    std::vector<std::pair<std::string, safetensors::Entry>> all(t.begin(), t.end());
                    if (a.w[0] == "run") safetensors::write(a.w[2], all); // an echo: what a round trip through this reader and writer leaves
                    std::printf("line %zu: %s, %zu tensors\n", a.line, a.w[0].c_str(), all.size());
                    files++;
                } else std::printf("line %zu: %s\n", a.line, a.w[0].c_str());
            }
            std::printf("script ok: %zu actions, %zu files read\n", script.size(), files);
            return 0;
        }
        line = 0;
        const onnx::Model m = onnx::load(argv[1]);
        Context ctx(0);
        ctx.enable_pool();
        Graph g(ctx, m);
        for (auto &s : g.step_names()) std::printf("step %s\n", s.c_str());
        std::map<std::string, std::vector<Tensor>> held;
        FeedSet captured;
        for (auto &a : script) {
            line = a.line; what = a.w[0];
            if (what == "run") {
                FeedSet fs;
                load_feeds(ctx, g, a.w[1], fs, false);
                const std::vector<Tensor> outs = g.run(fs.feeds);
                ctx.sync();
                save_outputs(ctx, g, outs, a.w[2]);
            } else if (what == "hold") {
                FeedSet fs;
                load_feeds(ctx, g, a.w[1], fs, false);
                held[a.w[2]] = g.run(fs.feeds);
                ctx.sync();
            } else if (what == "read") {
                auto it = held.find(a.w[1]);
                if (it == held.end()) throw GraphError("no held run tagged " + a.w[1]);
                {
                    // (steps + 1) buffers of every held output's byte size, all alive at once, empty the pool's list for that size: whatever any run left there
                    // is handed out and filled (graph_outputs_outlive_run.cpp)
                    std::vector<Tensor> scribble;
                    for (size_t round = 0; round < g.num_steps() + 1; round++)
                        for (auto &kv : held)
                            for (auto &o : kv.second) {
                                if (!o.bytes()) continue;
                                scribble.emplace_back(ctx, std::vector<int64_t>{(int64_t)o.bytes()}, DType::U8);
                                ctx.check(rten_hip_memset(ctx.raw(), scribble.back().ptr(), 0xA5, o.bytes()));
                            }
                    ctx.sync();
                }
                save_outputs(ctx, g, it->second, a.w[2]);
            } else if (what == "distinct") {
                auto x = held.find(a.w[1]), y = held.find(a.w[2]);
                if (x == held.end() || y == held.end()) throw GraphError("no held run tagged " + (x == held.end() ? a.w[1] : a.w[2]));
                for (size_t i = 0; i < x->second.size(); i++)
                    for (size_t j = 0; j < y->second.size(); j++)
                        if (x->second[i].ptr() && x->second[i].ptr() == y->second[j].ptr())
                            throw GraphError("output " + g.outputs()[i].name + " of " + a.w[1] + " and output " + g.outputs()[j].name + " of " + a.w[2] + " share one device address");
            } else if (what == "capture") {
                FeedSet fs; // the previous capture's feeds stay until Graph::capture has released the graph that reads them
                load_feeds(ctx, g, a.w[1], fs, false);
                g.capture(fs.feeds);
                captured = std::move(fs);
                g.replay();
                ctx.sync();
                save_outputs(ctx, g, g.captured_outputs(), a.w[2]);
            } else if (what == "refill") {
                load_feeds(ctx, g, a.w[1], captured, true);
            } else if (what == "replay") {
                g.replay();
                ctx.sync();
                save_outputs(ctx, g, g.captured_outputs(), a.w[1]);
            } else if (what == "tune") {
                FeedSet fs;
                load_feeds(ctx, g, a.w[1], fs, false);
                std::printf("line %zu: tuned %zu steps\n", a.line, g.autotune(fs.feeds, 1));
            } else if (what == "shape-plans") {
                g.set_shape_plans(read_plan_table(a.w[1]));
            } else if (what == "plan") {
                std::printf("line %zu: %zu steps took an entry\n", a.line, g.apply_plan(read_plan_table(a.w[1])));
            }
        }
        ctx.sync();
        std::printf("ran %zu actions on %zu steps, %zu by a shape-keyed plan\n", script.size(), g.num_steps(), g.num_shape_planned());
        return 0;
    } catch (const OpError &e) {
        std::fprintf(stderr, "error: %s%s\n", line ? ("line " + std::to_string(line) + " (" + what + "): ").c_str() : "", e.what());
        return e.kind == OpError::BackendUnavailable ? 2 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s%s\n", line ? ("line " + std::to_string(line) + " (" + what + "): ").c_str() : "", e.what());
        return 1;
    }
}
