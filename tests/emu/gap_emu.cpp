// A host execution of the LONG form of the device gap aligner.  This file compiles parsnp_amd/csrc/engine/gapalign_hip.hip itself,
// unchanged, for the host (tests/emu/hipstub/hip/hip_runtime.h stands in for the HIP runtime; same -ffp-contract=off as the
// product's build) and runs pm_gap_align_groups_long -> align_groups -> gap_align_long_kernel as they are: one workgroup at a
// time, 256 lanes.
//
// A lane is a fiber.  It runs until it reaches a point where the device's lanes meet -- GA_SYNC (__syncthreads), GA_WAVE_SYNC (the
// wave barrier), a shuffle or a ballot -- and the scheduler below then runs the next lane.  A wavefront runs on (through its own
// wave-level meeting points) until all its lanes stand at a workgroup barrier, then the next wavefront runs; when all four stand
// there, all go on.  Two schedules: ascending (wavefront 0..3, lane 0..63 between two meeting points) and descending (wavefront
// 3..0, lane 63..0: gap_emu_set_schedule(1) or PM_GAP_EMU_REVERSE=1, the counterpart of PM_EMU_REVERSE_WAVES).  Code that is
// correct on the device gives the same rows under both; a barrier missing between two wavefronts, or between the lanes of one,
// makes one of them read what the other has not written yet (or has already overwritten) under one of the two.
//
// SCOPE: the long form only.  The one-wavefront forms (narrow, wide, tall: gap_align_kernel) rely on the lockstep of a wavefront
// without a fence -- the narrow re-spelling has "every lane reads ... before any lane writes" -- and a lane-at-a-time execution of
// them would be unfaithful.  A launch of anything but 256 threads is refused (the call returns PM_EHIP), so calls given to this
// library hold long jobs only: every job has a string of more than 320 bases, or is declined on the host before any launch.
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>

gap_emu_idx threadIdx, blockIdx;
hipError_t gap_emu_last_error = hipSuccess;

namespace gap_emu {
constexpr int kLanes = 256, kStack = 256 * 1024;
enum { kRunnable = 0, kDone = 3 };
struct Fiber { void* sp; int kind; };
Fiber fibers[kLanes];
void* sched_sp;
int cur = -1, live_threads = 0, reverse = 0;
uint32_t exchange[4][2][64];
int parity[kLanes];
const std::function<void()>* body;
std::vector<uint8_t> stacks;

#if defined(__x86_64__)
// save the callee-saved registers on the running stack, leave its pointer in *save, take the other stack
extern "C" void gap_emu_switch(void** save, void* to);
asm(".text\n.globl gap_emu_switch\n.type gap_emu_switch,@function\ngap_emu_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n  ret\n"
    ".size gap_emu_switch,.-gap_emu_switch\n");
#else
#error "tests/emu/gap_emu.cpp switches fibers with x86-64 code"
#endif

void entry() {
    (*body)();
    fibers[cur].kind = kDone;
    gap_emu_switch(&fibers[cur].sp, sched_sp);
    abort();
}
void prepare(int t) {
    uint8_t* top = stacks.data() + (size_t)(t + 1) * kStack;
    top -= (uintptr_t)top & 15;
    void** sp = (void**)(top - 16);
    *sp = (void*)&entry;              // the `ret` of the first switch lands here with the stack as after a call
    sp -= 6;
    for (int k = 0; k < 6; k++) sp[k] = nullptr;
    fibers[t].sp = sp; fibers[t].kind = kRunnable; parity[t] = 0;
}
void resume(int t) {
    cur = t; threadIdx.x = (unsigned)t;
    gap_emu_switch(&sched_sp, fibers[t].sp);
    cur = -1;
}
[[noreturn]] void die(const char* what) { fprintf(stderr, "gap_emu: %s\n", what); abort(); }

// one workgroup
void run_block() {
    const int waves = live_threads / 64;
    for (int t = 0; t < live_threads; t++) prepare(t);
    for (;;) {
        int waves_done = 0;
        for (int wi = 0; wi < waves; wi++) {
            const int w = reverse ? waves - 1 - wi : wi;
            for (;;) {
                int at_wave = 0, at_block = 0, done = 0;
                for (int li = 0; li < 64; li++) {
                    const int t = w * 64 + (reverse ? 63 - li : li);
                    if (fibers[t].kind != kDone) resume(t);
                    at_wave += fibers[t].kind == GAP_EMU_WAVE; at_block += fibers[t].kind == GAP_EMU_BLOCK; done += fibers[t].kind == kDone;
                }
                if (done == 64) { waves_done++; break; }
                if (at_wave && at_block) die("the lanes of a wavefront stand at a wave-level and at a workgroup-level meeting point at once");
                if (at_block) { if (done) die("lanes of a wavefront returned while others wait at a workgroup barrier"); break; }
            }
        }
        if (waves_done == waves) return;
        if (waves_done) die("a wavefront returned while others wait at a workgroup barrier");
    }
}
}  // namespace gap_emu

void gap_emu_yield(int kind) {
    using namespace gap_emu;
    if (cur < 0) die("a meeting point outside a launch");
    fibers[cur].kind = kind;
    const int t = cur;
    gap_emu_switch(&fibers[t].sp, sched_sp);
}
uint32_t* gap_emu_exchange() {
    using namespace gap_emu;
    const int p = parity[cur]; parity[cur] ^= 1;
    return exchange[cur >> 6][p];
}
int gap_emu_lane_live(int lane) { return gap_emu::fibers[(gap_emu::cur & ~63) + lane].kind != gap_emu::kDone; }
int gap_emu_launch(unsigned blocks, unsigned threads, const std::function<void()>& fn) {
    using namespace gap_emu;
    if (threads != kLanes) return hipErrorInvalidValue;      // SCOPE above
    if (stacks.empty()) stacks.resize((size_t)kLanes * kStack + 16);
    const char* e = getenv("PM_GAP_EMU_REVERSE");
    if (e && *e) reverse = atoi(e) != 0;
    body = &fn; live_threads = (int)threads;
    for (unsigned b = 0; b < blocks; b++) { blockIdx.x = b; run_block(); }
    body = nullptr;
    return hipSuccess;
}
// 0: ascending, 1: descending (PM_GAP_EMU_REVERSE, when set, overrides it at every launch)
extern "C" void gap_emu_set_schedule(int descending) { gap_emu::reverse = descending != 0; }

#include "../../parsnp_amd/csrc/engine/gapalign_hip.hip"
