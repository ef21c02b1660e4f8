// ttt_engine.h — the TicTacToe engine and net handles (ttt.hip), shared with
// the TicTacToe learner (ttt_learner.hip on learner_common.h's shared core),
// which runs on the engine's device and stream and refreshes a net's weights
// in place.
#pragma once
#include "spai_internal.h"

namespace spai {
namespace ttt {

constexpr int kCells = 9;
constexpr int kHid = 64;
constexpr int kMaxBlocks = 16;

struct State {
    uint16_t x, o;
    uint8_t n, status;
};

struct Engine {
    int device = 0;
    spai_config cfg{};
    hipStream_t stream = nullptr;
    DevBuf<State> slots;
    uint32_t n_slots = 0;
    DevBuf<int32_t> si;
    DevBuf<uint32_t> su;
    DevBuf<float> sf, sf2;
    // trees
    uint32_t n_trees = 0, cap = 0;
    DevBuf<uint4> nodes;
    DevBuf<uint32_t> root, next_free, path, depth, active, counts, err, stats, pick;
    DevBuf<State> root_state, leaf, adv;
    DevBuf<uint32_t> btree;
    DevBuf<float> bx, blogits, bvalue;
    struct Net *net = nullptr;
};

struct Net {
    Engine *eng = nullptr;
    int blocks = 0;
    DevBuf<float> wt, b, pl_w, pl_b, vl_w, vl_b;
    DevBuf<float> io_x, io_l, io_v;
    uint32_t io_cap = 0;
};

inline size_t num_params(int blocks) {
    auto conv = [](size_t ci, size_t co) { return co * ci * 9 + co + 4 * co; };
    return conv(3, kHid) + (size_t)blocks * 2 * conv(kHid, kHid) + conv(kHid, 32) + 9 * 288 + 9 + conv(kHid, 3) +
           27 + 1;
}

}  // namespace ttt
}  // namespace spai

struct spai_ttt : spai::ttt::Engine {};
struct spai_ttt_net : spai::ttt::Net {};
