// TEST INFRASTRUCTURE: a HIP runtime that logs instead of executing.
//
// Defines exactly the runtime symbols libmacvo_hip's objects import, so that the library's host code — the frame driver above all — links into a
// stand-alone CPU program (pipe_trace.cpp) and every launch, event edge and copy it issues is printed in issue order: the driver's schedule as text.
// Streams and events are numbered in creation order.  Copies and memsets also execute (the "device" arena is host memory); kernels do not.
#include <hip/hip_runtime_api.h>

#include <cxxabi.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

struct ihipStream_t { int id; };
struct ihipEvent_t { int id; bool recorded; };

namespace {

struct Call { dim3 grid, block; size_t lds; hipStream_t stream; };

struct State {
    std::mutex mu;   // guards everything below (the driver's launch thread logs too)
    std::map<const void*, std::string> kernels;
    std::vector<std::string> log;
    const char* arena = nullptr;
    size_t arena_bytes = 0;
    int n_streams = 0, n_events = 0;
    bool query_ready = false;
};
State& st() {   // (the registration hooks run from static constructors: built on first use, never destroyed)
    static State* s = new State;
    return *s;
}
thread_local std::vector<Call> call_stack;

// "void ns::kernel<3, false>(float*, int)" -> "ns::kernel<3, false>"
std::string kernel_name(const char* mangled) {
    // (_Float16, "DF16_", is spelled as the older half type "Dh": demanglers that predate the former still print the name, as `half`; neither is a
    // substitution candidate, so the rest of the name is unaffected)
    std::string m = mangled;
    for (size_t at; (at = m.find("DF16_")) != std::string::npos;) m.replace(at, 5, "Dh");
    int rc = 0;
    char* d = abi::__cxa_demangle(m.c_str(), nullptr, nullptr, &rc);
    std::string s = (rc == 0 && d) ? d : mangled;
    free(d);
    static const std::string anon = "(anonymous namespace)::";
    for (size_t at; (at = s.find(anon)) != std::string::npos;) s.erase(at, anon.size());
    int depth = 0;
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] == '<') ++depth;
        else if (s[i] == '>') --depth;
        else if (s[i] == '(' && depth == 0) { s.resize(i); break; }
    }
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    return s;
}

std::string sname(hipStream_t s) { return s ? "S" + std::to_string(s->id) : std::string("S-"); }
std::string ename(hipEvent_t e) { return e ? "e" + std::to_string(e->id) : std::string("e-"); }
std::string pname(const State& S, const void* p) {
    if (!p) return "null";
    const char* c = (const char*)p;
    if (S.arena && c >= S.arena && c < S.arena + S.arena_bytes) return "A+" + std::to_string((size_t)(c - S.arena));
    return "host";
}
// A query answered "not ready" and the wait it leads to are one line, `wait_if_pending`; a query followed by anything else is a line of its own.
thread_local hipEvent_t queried = nullptr;
void flush_query(State& S) {
    if (queried) S.log.push_back("query " + ename(queried));
    queried = nullptr;
}
void say(State& S, const std::string& line) {
    flush_query(S);
    S.log.push_back(line);
}
std::string dims(dim3 d) {   // "(6,2)": trailing ones are left out
    std::string s = "(" + std::to_string(d.x);
    if (d.y != 1 || d.z != 1) s += "," + std::to_string(d.y);
    if (d.z != 1) s += "," + std::to_string(d.z);
    return s + ")";
}

}  // namespace

// ---- the harness's own controls (pipe_trace.cpp)
extern "C" void fake_hip_arena(const void* base, size_t bytes) {
    std::lock_guard<std::mutex> lk(st().mu);
    st().arena = (const char*)base;
    st().arena_bytes = bytes;
}
extern "C" void fake_hip_event_query_ready(int ready) {
    std::lock_guard<std::mutex> lk(st().mu);
    st().query_ready = ready != 0;
}
extern "C" void fake_hip_note(const char* text) {
    std::lock_guard<std::mutex> lk(st().mu);
    say(st(), text);
}
extern "C" void fake_hip_dump(FILE* f) {
    std::lock_guard<std::mutex> lk(st().mu);
    flush_query(st());
    for (const std::string& l : st().log) fprintf(f, "%s\n", l.c_str());
    st().log.clear();
}

// ---- registration and launch
extern "C" void** __hipRegisterFatBinary(const void*) {
    static void* handle = nullptr;
    return &handle;
}
extern "C" void __hipUnregisterFatBinary(void**) {}
extern "C" void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, uint3*, uint3*, dim3*, dim3*, int*) {
    std::lock_guard<std::mutex> lk(st().mu);
    st().kernels[host_fn] = kernel_name(device_name);
}
extern "C" hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    call_stack.push_back(Call{grid, block, lds, stream});
    return hipSuccess;
}
extern "C" hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    if (call_stack.empty()) return hipErrorInvalidValue;
    const Call c = call_stack.back();
    call_stack.pop_back();
    *grid = c.grid; *block = c.block; *lds = c.lds; *stream = c.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void**, size_t lds, hipStream_t s) {
    State& S = st();
    std::lock_guard<std::mutex> lk(S.mu);
    const auto it = S.kernels.find(fn);
    say(S, "launch " + sname(s) + " " + (it == S.kernels.end() ? std::string("?") : it->second) + " grid" + dims(grid) + " block" + dims(block) + " lds " +
               std::to_string(lds));
    return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void*, hipFuncAttribute, int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }

// ---- device
hipError_t hipGetDevice(int* dev) { *dev = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceProperties(hipDeviceProp_t* prop, int) {
    memset(prop, 0, sizeof(*prop));
    prop->multiProcessorCount = 256;   // (the MI355X's)
    return hipSuccess;
}
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 0; *hi = -1; return hipSuccess; }

// ---- streams
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned flags, int priority) {
    State& S = st();
    std::lock_guard<std::mutex> lk(S.mu);
    *s = new ihipStream_t{++S.n_streams};
    say(S, "stream_create " + sname(*s) + " flags " + std::to_string(flags) + " priority " + std::to_string(priority));
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    std::lock_guard<std::mutex> lk(st().mu);
    say(st(), "stream_destroy " + sname(s));
    delete s;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    std::lock_guard<std::mutex> lk(st().mu);
    say(st(), "stream_sync " + sname(s));
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    std::lock_guard<std::mutex> lk(st().mu);
    const bool conditional = queried == e;
    if (conditional) queried = nullptr;
    say(st(), (conditional ? "wait_if_pending " : "wait ") + sname(s) + " " + ename(e));
    return hipSuccess;
}

// ---- events (creation and destruction are not logged: the ids say when an event was made)
static hipError_t new_event(hipEvent_t* e) {
    std::lock_guard<std::mutex> lk(st().mu);
    *e = new ihipEvent_t{++st().n_events, false};
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) { return new_event(e); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return new_event(e); }
hipError_t hipEventDestroy(hipEvent_t e) { delete e; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    std::lock_guard<std::mutex> lk(st().mu);
    e->recorded = true;
    say(st(), "record " + sname(s) + " " + ename(e));
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    std::lock_guard<std::mutex> lk(st().mu);
    say(st(), "event_sync " + ename(e));
    return hipSuccess;
}
hipError_t hipEventQuery(hipEvent_t e) {   // "not ready" unless told otherwise, so that every conditional wait shows
    std::lock_guard<std::mutex> lk(st().mu);
    if (st().query_ready) {
        say(st(), "query " + ename(e) + " ready");
        return hipSuccess;
    }
    flush_query(st());
    queried = e;
    return hipErrorNotReady;
}
hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    std::lock_guard<std::mutex> lk(st().mu);
    say(st(), "elapsed " + ename(a) + " " + ename(b));
    if (!a || !b || !a->recorded || !b->recorded) return hipErrorInvalidHandle;
    *ms = 0.f;
    return hipSuccess;
}

// ---- memory
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) {
    *p = calloc(bytes ? bytes : 1, 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
static hipError_t copy(const char* what, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, const std::string& on) {
    State& S = st();
    std::lock_guard<std::mutex> lk(S.mu);
    say(S, std::string(what) + on + " " + pname(S, dst) + " <- " + pname(S, src) + " bytes " + std::to_string(bytes) + " kind " + std::to_string((int)kind));
    if (bytes) memmove(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { return copy("memcpy", dst, src, bytes, kind, ""); }
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    return copy("memcpy_async ", dst, src, bytes, kind, sname(s));
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
    State& S = st();
    std::lock_guard<std::mutex> lk(S.mu);
    say(S, "memset_async " + sname(s) + " " + pname(S, dst) + " value " + std::to_string(value) + " bytes " + std::to_string(bytes));
    if (bytes) memset(dst, value, bytes);
    return hipSuccess;
}
