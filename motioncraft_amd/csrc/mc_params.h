// Host-side weight storage shared by the library's native objects (the denoiser model and the four encoders):
//   ParamStore  named fp32 parameters in device memory, uploaded from the host by the objects' *_set_param calls, plus the
//               buffers an object derives from them at finalize (repacked / stacked weights)
//   Workspace   the grow-only scratch buffer of a step-invariant encoder's forward calls
// Each object keeps its own policy on top (when a weight may be replaced, what finalize derives).
#pragma once
#include "mc_common.h"
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

class ParamStore {
  public:
    // label: the owner's name, prefixed to every lookup error ("" = none)
    explicit ParamStore(const char* label) : prefix_(*label ? std::string(label) + ": " : std::string()) {}
    ParamStore(const ParamStore&) = delete;
    ParamStore& operator=(const ParamStore&) = delete;
    ~ParamStore() {
        for (auto& kv : params_) (void)hipFree(kv.second.data);
        clear_derived();
    }

    // upload `numel` floats from the host under `name` (synchronous); a parameter of that name is replaced only once the new
    // copy is complete, and a failed copy frees the new buffer
    int set(const std::string& name, const float* host, int64_t numel) {
        float* d = nullptr;
        MC_HIP(hipMalloc((void**)&d, (size_t)numel * sizeof(float)));
        const hipError_t e = hipMemcpy(d, host, (size_t)numel * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            mc_set_error("%sparameter '%s': host-to-device copy failed: %s", prefix_.c_str(), name.c_str(), hipGetErrorString(e));
            return MC_ERR_HIP;
        }
        Param& p = params_[name];
        if (p.data) (void)hipFree(p.data);
        p = {d, numel};
        return MC_OK;
    }

    // the device address of parameter `name`, which must hold `numel` floats (MC_ERR_STATE otherwise)
    int get(const std::string& name, int64_t numel, const float** out) const {
        auto it = params_.find(name);
        if (it == params_.end()) {
            mc_set_error("%smissing parameter '%s'", prefix_.c_str(), name.c_str());
            return MC_ERR_STATE;
        }
        if (it->second.numel != numel) {
            mc_set_error("%sparameter '%s' has %ld elements, expected %ld", prefix_.c_str(), name.c_str(), (long)it->second.numel,
                         (long)numel);
            return MC_ERR_STATE;
        }
        *out = it->second.data;
        return MC_OK;
    }

    // get() of each entry in order, up to the first failure
    struct Ref {
        const float** out;
        std::string name;
        int64_t numel;
    };
    int bind(std::initializer_list<Ref> refs) const {
        for (const Ref& p : refs)
            if (int r = get(p.name, p.numel, p.out)) return r;
        return MC_OK;
    }

    bool has(const std::string& name) const { return params_.count(name) != 0; }

    // a device buffer of `floats` floats that lives until the next clear_derived() or the store's destruction
    int derived(size_t floats, float** out) {
        MC_HIP(hipMalloc((void**)out, floats * sizeof(float)));
        derived_.push_back(*out);
        return MC_OK;
    }

    void clear_derived() {
        for (float* p : derived_) (void)hipFree(p);
        derived_.clear();
    }

  private:
    struct Param {
        float* data = nullptr;
        int64_t numel = 0;
    };
    std::string prefix_;
    std::map<std::string, Param> params_;
    std::vector<float*> derived_;
};

struct Workspace {
    float* buf = nullptr;
    size_t floats = 0;

    Workspace() = default;
    Workspace(const Workspace&) = delete;
    Workspace& operator=(const Workspace&) = delete;
    ~Workspace() {
        if (buf) (void)hipFree(buf);
    }

    // at least `n` floats in `buf`; growing waits for `s` (earlier launches may still read the old buffer) and reallocates
    int ensure(size_t n, hipStream_t s) {
        if (n <= floats) return MC_OK;
        if (buf) {
            MC_HIP(hipStreamSynchronize(s));
            MC_HIP(hipFree(buf));
            buf = nullptr;
            floats = 0;
        }
        MC_HIP(hipMalloc((void**)&buf, n * sizeof(float)));
        floats = n;
        return MC_OK;
    }
};
