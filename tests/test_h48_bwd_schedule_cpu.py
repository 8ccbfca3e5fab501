"""Block schedule of the one-trial H = 48 backward, replayed on the host.  No GPU needed.

nsd_ring_block.h holds the decisions "does this block of 8 macro steps run without its tests" as host/device constexpr helpers
(namespace h48_bwd_sched); the roles of nsd_lstm2_bwd48.hip call them.  A stand-alone host program walks every role's loop
skeleton with those helpers for T = 1 .. 1100 and checks that

  * every role covers each macro step exactly once and runs exactly the chains' number of step barriers per trial (one more or
    one fewer in any role hangs the workgroup);
  * no untested block holds a step at which one of the tests it leaves out would have gone the other way: the window tests of the
    recurrences, `m >= 4` / `t > 0` / `t == T - 1` / the dx range of the x1 waves, `m >= 1` and the da range of the converters,
    `m >= 17` of the tiles.  (The loader keeps the range test of its pieces.)
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neural-speech-decoding_amd", "csrc")

PROGRAM = r"""
#include "nsd_ring_block.h"
#include <cstdio>
#include <vector>
using namespace h48_bwd_sched;

static long fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (fails++ < 20) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } } while (0)
static bool in_range(int t, int T) { return t >= 0 && t < T; }

struct Walk {
    std::vector<int> hit; int barriers = 1;           // the barrier in front of the first step
    explicit Walk(int n) : hit(n, 0) {}
    void step(int m) { if (m >= 0 && m < (int)hit.size()) ++hit[m]; else ++fails; ++barriers; }
    void done(const char *role, int T, int want) {
        for (size_t m = 0; m < hit.size(); ++m) CHECK(hit[m] == 1, "%s T=%d: step %zu covered %d times", role, T, m, hit[m]);
        CHECK(barriers == want, "%s T=%d: %d barriers, the chains run %d", role, T, barriers, want);
    }
};

int main() {
    for (int T = 1; T <= 1100; ++T) {
        const int n = n_steps(T);
        CHECK(n % 16 == 0 || n % 16 == 8, "T=%d: n_steps %d", T, n);
        CHECK(n > tbase(0, T) + 1, "T=%d: n_steps %d does not reach layer 0's last step and the hand-off behind it", T, n);
        const int want = 1 + n;
        // recurrences
        for (int layer = 0; layer < 2; ++layer) {
            Walk w(n);
            for (int m0 = 0; m0 < n; m0 += BLOCK) {
                const bool in = chain_inside(layer, T, m0);
                for (int k = 0; k < BLOCK; ++k) {
                    const int t = tbase(layer, T) - (m0 + k);
                    if (in) CHECK(in_range(t, T) && in_range(t + 1, T), "chain%d T=%d m=%d untested, t=%d", layer, T, m0 + k, t);
                    w.step(m0 + k);
                }
            }
            w.done(layer ? "chain1" : "chain0", T, want);
        }
        // x1 waves: ring blocks of 8
        for (int duty = X1_PREP1; duty <= X1_DX; ++duty) {
            Walk w(n);
            for (int m0 = 0; m0 < n; m0 += BLOCK) {
                const bool in = x1m_inside(duty, T, m0);
                for (int k = 0; k < BLOCK; ++k) {
                    const int m = m0 + k;
                    if (in) {
                        if ((k & 3) == 0) CHECK(m >= 4, "x1 duty %d T=%d m=%d: hand-off before step 4", duty, T, m);
                        if (duty == X1_PREP1 || duty == X1_PREP0) {
                            const int t = tbase(duty == X1_PREP1 ? 1 : 0, T) - (m + 1);
                            CHECK(t > 0 && t != T - 1, "x1 duty %d T=%d m=%d: prep of t=%d untested", duty, T, m, t);
                        }
                        if (duty == X1_DX) CHECK(m >= 1 && in_range(T + 2 + DL0 - m, T), "x1 dx T=%d m=%d: t0=%d untested", T, m, T + 2 + DL0 - m);
                    }
                    w.step(m);
                }
            }
            w.done("x1", T, want);
        }
        // dW waves: the first 16 steps (FIRST half: no tiles; a converter tests every step), then 16-step trips -- the half with tiles
        // untested while the helper says so (one loop), tested from there on (a second loop); a half without tiles chooses per half
        for (int duty = 0; duty < 6; ++duty) {
            const bool conv = duty >= 4;
            const int cl = 5 - duty;
            Walk w(n);
            auto half = [&](int m0, int ph, bool first, bool inside) {
                CHECK((m0 & 15) == ph, "dW%d T=%d: half at %d compiled for phase %d", duty, T, m0, ph);
                for (int k = 0; k < BLOCK; ++k) {
                    const int m = m0 + k, p = ph + k;
                    const bool tile_step = p >= 1 && p <= 5;
                    if (tile_step && first) CHECK(m < 17, "dW%d T=%d m=%d: a tile skipped", duty, T, m);
                    if (tile_step && !first) CHECK(m >= 17 && dw_tiles(m0), "dW%d T=%d m=%d: a tile before its window", duty, T, m);
                    if (conv && inside) CHECK(m >= 1 && in_range(tbase(cl, T) - (m - 1), T), "dW%d T=%d m=%d: da outside the trial untested", duty, T, m);
                    w.step(m);
                }
            };
            auto second_half = [&](int m0) { half(m0, 8, false, conv ? dw_conv_inside(cl, T, m0) : true); };
            int m0 = 0;
            half(m0, 0, true, !conv);
            if (8 < n) second_half(m0 + 8);
            m0 += 16;
            for (; m0 < n && (!conv || dw_conv_inside(cl, T, m0)); m0 += 16) {
                half(m0, 0, false, true);
                if (m0 + 8 < n) second_half(m0 + 8);
            }
            if (conv)
                for (; m0 < n; m0 += 16) {
                    half(m0, 0, false, false);
                    if (m0 + 8 < n) second_half(m0 + 8);
                }
            w.done("dW", T, want);
        }
        // loader: whole chunks of 8, every piece tested
        {
            Walk w(n);
            for (int m0 = 0; m0 < n; m0 += BLOCK)
                for (int k = 0; k < BLOCK; ++k) w.step(m0 + k);
            w.done("loader", T, want);
        }
        // the steady state exists: a long trial runs most blocks untested in every role
        if (T >= 64) {
            int un = 0;
            for (int m0 = 0; m0 < n; m0 += BLOCK)
                un += chain_inside(1, T, m0) && chain_inside(0, T, m0) && x1m_inside(X1_PREP1, T, m0) && x1m_inside(X1_PREP0, T, m0) &&
                      x1m_inside(X1_DX, T, m0) && dw_conv_inside(1, T, m0) && dw_conv_inside(0, T, m0);
            CHECK(un >= n / BLOCK - 4, "T=%d: only %d of %d blocks untested in every role", T, un, n / BLOCK);
        }
    }
    std::printf("%ld failures\n", fails);
    return fails ? 1 : 0;
}
"""


def test_every_role_walks_the_chains_schedule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "sched.cpp", tmp_path / "sched"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("0 failures")
