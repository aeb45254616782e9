// dev_pool.h — one owner for what a context allocates: device memory, pinned host memory, events
// and streams.  The pool records every resource it hands out and drops them all when it is
// destroyed: memory first, then events, then streams, each kind newest first.  Plain host C++ (no
// HIP types): the runtime is reached through the caller's PoolBackend, so the CPU suite drives the
// same code with a counting backend that fails on demand (oracle/dev_pool_check.cpp).
#pragma once
#include <cstddef>
#include <initializer_list>
#include <vector>

namespace vo {

enum PoolKind { POOL_DEVICE, POOL_PINNED, POOL_EVENT, POOL_STREAM };

// make: 0 and the handle in *out, or the runtime's error code (*out untouched).  bytes is 0 for
// events and streams.
struct PoolBackend {
    int (*make)(PoolKind kind, size_t bytes, void** out);
    void (*drop)(PoolKind kind, void* handle);
};

class DevPool {
public:
    // one request of group() / grow(): the caller's pointer and the bytes it is to address
    struct Req { void** p; size_t bytes; };
    template <class T> static Req req(T*& p, size_t count) { return {(void**)&p, sizeof(T) * count}; }

    explicit DevPool(const PoolBackend& be) : be_(be) {}
    DevPool(const DevPool&) = delete;
    DevPool& operator=(const DevPool&) = delete;
    ~DevPool()
    {
        for (int pass = 0; pass < 3; ++pass)
            for (size_t k = own_.size(); k-- > 0;)
                if (teardown_pass(own_[k].kind) == pass) be_.drop(own_[k].kind, own_[k].handle);
    }

    // Every call returns 0 or the backend's error code; after a failure the caller's pointer is
    // as it was.  Events and streams are the runtime's opaque pointer handles.
    template <class T> int alloc(T*& p, size_t count) { return make(POOL_DEVICE, sizeof(T) * count, (void**)&p); }
    template <class T> int pinned(T*& p, size_t count) { return make(POOL_PINNED, sizeof(T) * count, (void**)&p); }
    template <class H> int event(H*& e) { return make(POOL_EVENT, 0, (void**)&e); }
    template <class H> int stream(H*& s) { return make(POOL_STREAM, 0, (void**)&s); }

    // Device buffers, all or nothing: every pointer (null on entry) is set, or none is and nothing
    // of the group stays allocated.
    int group(std::initializer_list<Req> reqs)
    {
        const size_t mark = own_.size();
        for (const Req& r : reqs) {
            const int rc = make(POOL_DEVICE, r.bytes, r.p);
            if (rc == 0) continue;
            while (own_.size() > mark) { be_.drop(own_.back().kind, own_.back().handle); own_.pop_back(); }
            for (const Req& q : reqs) *q.p = nullptr;
            return rc;
        }
        return 0;
    }

    // Replace the buffers of reqs by new ones of the requested sizes, all or nothing (a failure
    // leaves the old ones in place).  The old ones are released at once, or, with `retired`,
    // appended to it still owned: the caller releases them once nothing reads them any more.
    int grow(std::initializer_list<Req> reqs, std::vector<void*>* retired = nullptr)
    {
        std::vector<void*> old;
        for (const Req& r : reqs) { old.push_back(*r.p); *r.p = nullptr; }
        const int rc = group(reqs);
        size_t k = 0;
        for (const Req& r : reqs) {
            void* o = old[k++];
            if (rc) *r.p = o;
            else if (o && retired) retired->push_back(o);
            else release(o);
        }
        return rc;
    }

    // Free one resource early and null the caller's pointer.  Null, or a pointer the pool does not
    // own (already released, say), is left alone.
    template <class T> void release(T*& p)
    {
        for (size_t k = own_.size(); k-- > 0;)
            if (p && own_[k].handle == (void*)p) {
                be_.drop(own_[k].kind, own_[k].handle);
                own_.erase(own_.begin() + k);
                p = nullptr;
                return;
            }
    }

    size_t live() const { return own_.size(); }

private:
    struct Owned { PoolKind kind; void* handle; };
    static int teardown_pass(PoolKind k) { return k == POOL_STREAM ? 2 : k == POOL_EVENT ? 1 : 0; }
    int make(PoolKind kind, size_t bytes, void** out)
    {
        void* h = nullptr;
        const int rc = be_.make(kind, bytes, &h);
        if (rc) return rc;
        own_.push_back({kind, h});
        *out = h;
        return 0;
    }
    PoolBackend be_;
    std::vector<Owned> own_;
};

}  // namespace vo
