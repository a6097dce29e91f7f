// yk_staging.h — the staged arrays of one host-array entry point: the caller's inputs copied to the device, temporaries,
// and outputs copied back.  Library-private; the only code that indexes yk_context::scratch.
//
// The rule that makes the slots safe.  Slots are reused from call to call, and the render loop may still be in flight on the
// context's streams when a call returns.  Reuse is safe because every user enqueues on ctx->stream — stream order covers it —
// and because DevBuf::ensure grows through hipFree, which waits for the device.  So a Staging takes no stream argument, and
// the `_device` entry points on a caller's stream use none of this: they never staged anything.  At most one Staging is live
// per context: the lock (YK_LOCK, taken before it is made) guarantees that between threads, and within a thread nothing
// called under a Staging makes another — what the render loop keeps on the device are named members of the context.
//
//     YK_LOCK(ctx);
//     Staging sg(ctx);
//     const float* d_in = sg.upload(in, n);       // slots in the order asked, copies in the order asked
//     float* d_out = sg.output(out, n);
//     if (!sg.ok()) return sg.status();           // before the first launch: a failed slot is a null pointer
//     launch(sg.stream, d_in, d_out);
//     sg.check(hipGetLastError());
//     return sg.finish();                         // the downloads in registration order, one synchronisation
// or, where the device work is one enqueue function, the last four lines as
//     return sg.run([&] { return enqueue(ctx, sg.stream, d_in, d_out); });
#pragma once
#include "yk_internal.h"

struct Staging {
    yk_context* const ctx;
    const hipStream_t stream;  // ctx->stream, for the launches and for a copy the helper does not know about

    explicit Staging(yk_context* c) : ctx(c), stream(c->stream) { (void)hipSetDevice(c->device); }
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;

    // `count` elements of a host array on the device; host NULL or count 0 only reserves the buffer
    template <class T> T* upload(const T* host, size_t count) {
        void* d = take(count * sizeof(T));
        if (d && host && count) check(hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, stream));
        return ok() ? static_cast<T*>(d) : nullptr;
    }
    // a temporary of `count` elements
    template <class T> T* temp(size_t count) { return static_cast<T*>(take(count * sizeof(T))); }
    // `count` elements finish() copies to `host`; host NULL: no slot, NULL (an output the caller did not ask for)
    template <class T> T* output(T* host, size_t count) {
        if (!host) return nullptr;
        void* d = take(count * sizeof(T));
        if (d) outs[n_outs++] = Out{host, d, count * sizeof(T)};
        return static_cast<T*>(d);
    }
    // uploaded now, copied back by finish()
    template <class T> T* inout(T* host, size_t count) {
        T* d = upload(host, count);
        if (d) outs[n_outs++] = Out{host, d, count * sizeof(T)};
        return d;
    }

    // the first device error sticks: later operations do nothing and return NULL
    void check(hipError_t e) {
        if (err == hipSuccess) err = e;
    }
    bool ok() const { return err == hipSuccess; }
    yk_status status() const {
        if (ok()) return YK_OK;
        return fail(ctx, err == hipErrorOutOfMemory ? YK_ERR_OUT_OF_MEMORY : YK_ERR_DEVICE, std::string("staged call: ") + hipGetErrorString(err));
    }
    // the registered downloads, enqueued in registration order (for a call that has a copy of its own to place after them)
    void download() {
        for (unsigned k = 0; k < n_outs && ok(); ++k) check(hipMemcpyAsync(outs[k].host, outs[k].dev, outs[k].bytes, hipMemcpyDeviceToHost, stream));
        n_outs = 0;
    }
    // download(), then the call's one synchronisation
    yk_status finish() {
        download();
        if (ok()) check(hipStreamSynchronize(stream));
        return status();
    }
    // The tail of an entry point whose device work is one call: nothing runs when a slot failed; a failure of enqueue()
    // (which returns a yk_status) is the call's, with no download and no synchronisation; otherwise finish().
    template <class Enqueue> yk_status run(const Enqueue& enqueue) {
        if (!ok()) return status();
        if (yk_status s = enqueue()) return s;
        return finish();
    }

private:
    static constexpr unsigned N_SLOTS = sizeof(yk_context::scratch) / sizeof(DevBuf);
    struct Out {
        void* host;
        const void* dev;
        size_t bytes;
    };
    Out outs[N_SLOTS];
    unsigned n_slots = 0, n_outs = 0;
    hipError_t err = hipSuccess;

    void* take(size_t bytes) {  // the next slot, grown to hold `bytes` (never smaller than 16 bytes)
        if (ok() && n_slots == N_SLOTS) err = hipErrorInvalidValue;  // more arrays than slots: a mistake in the entry point
        if (!ok()) return nullptr;
        DevBuf& b = ctx->scratch[n_slots++];
        check(b.ensure(std::max<size_t>(bytes, 16)));
        return ok() ? b.p : nullptr;
    }
};
