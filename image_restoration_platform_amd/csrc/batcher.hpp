// batcher.hpp -- the async batcher behind ire_submit / ire_poll / ire_job_release: restoreBatch's in-flight promises
// (server-node/src/services/restorator.js:181-236) and the worker's five concurrent jobs (design.md:851) coalesced into engine
// batches of up to max_batch equal-shape images.
//
// The state machine is a template over its BACKEND -- everything that touches the device (pinned / device staging, copies, the
// restore call, completion events) -- so that the same code is built twice: api.cpp instantiates it over HIP (HipBatchBackend),
// tests/native/batcher_*_stress.cpp over a host-only stub (batcher_stub.hpp) and run it under ThreadSanitizer and AddressSanitizer on the CPU box
// (sanitizers on the CPU build).  The stub is test infrastructure: libire.so never contains it.
//
// Data path, ONE host copy per direction: submit copies the caller's pixels straight into the pinned staging slot of the batch
// being gathered (in the caller's thread: concurrent callers copy concurrently), poll copies from the batch's pinned output to
// the caller (again in the caller's thread).
//
// A slot is FREE -> OPEN (gathering: submits reserve an index and stage into it; the launcher issues each staged image's H2D
// copy at once, under the previous batch's compute) -> CLOSED (launching) -> INFLIGHT (kernels + D2H enqueued) -> DONE (results
// in pin_out, waiting for its jobs' polls) -> FREE.  Two service threads: the launcher decides when a gathering batch goes, the
// completer waits for the oldest in-flight batch (first its compute, which wakes the launcher, then its D2H) and completes its
// jobs.  Every wait is on a condition variable with a deadline that means something (the linger bounds) -- no polling loops.
//
// When a batch goes: at once when it is full (the stream runs it behind the previous batch: no bubble); otherwise it keeps
// gathering while the GPU still computes the previous batch (launching then would only split what a closed-loop caller -- 3 jobs
// per restoreBatch, 5 per worker -- is about to resubmit), and when the GPU is idle after a short bounded linger: kLingerQuietUs
// after the last arrival, at most kLingerMaxUs after the first.
//
// A slot gathers jobs of ONE SlotKey: the images' size, the kind of job (pixel, file, upload, fusion) and what tells two slots of that kind
// apart -- a fusion job's number of views k, an upload's (stored h, stored w, orientation, max_dim).  The key also says how large a job's
// place in the slot's input is (in_bytes) and how many image places it takes: a fusion job's k views take k consecutive ones, so such a
// slot holds max_batch / k jobs (at most kGroupMaxJobs: a full slot is ONE fused launch) and closes by the same full / linger rules.  An
// upload job is a file job whose decoded image is oriented and fitted on the device before the network sees it: its h, w are the FITTED
// size, the rest of its key says how the backend gets there, and two keys never share a slot even where they give one fitted size.
//
// Every submit goes through ONE staging path (Batcher::stage): a place for the job, then its input written there in the caller's thread.
//
// A job handle is used by ONE thread at a time (poll it, or release it).  A timed-out poll leaves the job pending; the caller
// polls again or RELEASES it (the reference retries 3x on exactly this path: utils/retry.js:12-47): an abandoned job's slot
// position is still computed with its batch, but nobody is counted as waiting for it.
#pragma once
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "errors.hpp"

namespace ire {

constexpr int kSlots = 8;             // gathering | computing | up to six waiting for their polls (a caller that submits a burst before its first poll)
constexpr int kSlotsEager = 3;        // staging allocated at the first job of a shape; the other slots get theirs when first needed
constexpr int kLingerQuietUs = 250, kLingerMaxUs = 1500;
constexpr int kMaxBatch = 64;
constexpr int kGroupMaxJobs = 16;     // fusion jobs of one batch at most: what one fused launch takes (fusion.hpp kFuseMaxSets; api.cpp asserts that they agree)

enum class JobKind { Pixels, File, Upload, Group };
// What a slot gathers, and what a job is: jobs share a slot exactly when their keys are equal.
struct SlotKey {
    int h = 0, w = 0;                 // of every image of the job (an upload's: the FITTED size)
    JobKind kind = JobKind::Pixels;
    int k = 0;                        // Group: the job's views (2..3), staged one behind the other; else 0: one image
    int up[4] = {};                   // Upload: stored h, stored w, orientation, max_dim; else zeros
    bool operator==(const SlotKey& o) const { return h == o.h && w == o.w && kind == o.kind && k == o.k && !std::memcmp(up, o.up, sizeof(up)); }
    int images_per_job() const { return std::max(1, k); }
    size_t image_bytes() const { return (size_t)h * w * 3; }
    size_t in_bytes() const { return image_bytes() * (size_t)images_per_job(); }      // one job's staged input: its place in pin_in
    bool decoded() const { return kind == JobKind::File || kind == JobKind::Upload; }     // the input is a file's scan, decoded on the device
};

struct BatchSlot;
struct Job {
    SlotKey key;
    bool staged = false;              // input bytes are in the slot's pinned buffer (or in `in` on the overflow path)
    bool abandoned = false;           // released while pending: its result is dropped when the batch completes
    uint8_t v_jpeg[3] = {}, v_has[3] = {};      // per image of the job (entry 0 alone unless it is a fusion job): is_jpeg, scores supplied
    double v_scores[3][7] = {};                 // ... and those scores
    std::shared_ptr<void> file;       // decoded kinds: what the backend's file_plan / upload_plan made of the file's head; the staged input is the scan, cut
    size_t file_used = 0;             // bytes of the staged input (0: staging failed, nothing to decode)
    BatchSlot* slot = nullptr;        // where the input was staged and the output will be; null: overflow (no free slot at submit) / evicted / fetched
    int idx = -1;
    std::vector<uint8_t> in, out;     // overflow input / evicted output only
    double scores[7] = {};            // the result's (a fusion job's: its view 0's), from the batch
    ire_timings t{};
    int status = -1;                  // -1 pending, else ire_status
    int stage_status = IRE_OK;        // a job whose staging failed after it had got its place: the status it completes with
    std::string err;
};

// Host-visible staging of a slot.  The backend allocates and frees it (reserve / release) and keeps its own device side in `impl`.
struct SlotBufs {
    uint8_t *pin_in = nullptr, *pin_out = nullptr, *pin_jp = nullptr;
    double *pin_sc = nullptr, *pin_sc_in = nullptr;
    size_t cap = 0;                   // bytes of pin_in / pin_out
    bool fixed = false;               // pin_jp / pin_sc / pin_sc_in (and the backend's events) exist
    void* impl = nullptr;
};

struct BatchSlot {
    enum State { FREE, OPEN, CLOSED, INFLIGHT, DONE } state = FREE;
    SlotBufs b;
    uint8_t has_sc[kMaxBatch] = {};
    std::vector<std::shared_ptr<Job>> jobs;   // index order = position in the batch
    SlotKey key;                          // what it gathers: never two kinds, two k or two upload keys
    int h2d_issued = 0;                   // jobs whose H2D copy (decoded kinds: whose decode) is already on the copy-in stream
    int unread = 0, reading = 0;          // DONE: jobs that have not fetched their output yet / polls copying right now
    std::chrono::steady_clock::time_point first_arrival, last_arrival;
    int status = IRE_OK;
    std::string err;
};

// Backend concept (HipBatchBackend in api.cpp; StubBackend in tests/native/batcher_stub.hpp).  Every hook is required: the product has one
// backend and it serves every kind of job.
//   int  max_batch() const;
//   size_t out_bytes(int h, int w) const;                      bytes of one job's result place (h * w * 3 pixels, or the text of an encoded image)
//   const uint8_t* result_view(const uint8_t* place, int h, int w, size_t* len) const;
//                                                              where a result's payload starts inside its place and how long it really is (a
//                                                              result whose size does not depend on the data: place, out_bytes(h, w)).  Required,
//                                                              not detected: the identity form is one line, a trait and its branch were more
//   void start();                                              first submit, batcher lock held: streams
//   void thread_enter(const char* role);                       at the top of a service thread: device, CPU affinity
//   void reserve(SlotBufs&, size_t bytes, int max_batch);      grow to `bytes` per direction; STRONG guarantee: on a throw the SlotBufs is as before
//   void release(SlotBufs&) noexcept;
//   void h2d(SlotBufs&, size_t off, size_t bytes);             async copy pin_in -> device, copy-in stream; throws Error
//   void launch(SlotBufs&, int njobs, const SlotKey&, const uint8_t* has_sc);
//                                                              flags + restore (Group: of all njobs * k views, then the fusion) + scores + D2H, all
//                                                              enqueued; throws Error.  Job i owns images [i * images_per_job(), ...) of the slot's
//                                                              input and of pin_jp / has_sc / pin_sc_in, and result place i; pin_sc[7 * i ..] = its
//                                                              scores (a fusion job's: its view 0's)
//   bool computing(SlotBufs&) noexcept;                        the launched batch's compute has not finished (non-blocking)
//   void wait_compute(SlotBufs&) noexcept;                     blocks until it has
//   void wait_done(SlotBufs&, ire_timings&);                   blocks until pin_out / pin_sc are complete; throws Error
//   void drain() noexcept;                                     after a failed launch: nothing enqueued may still touch a slot
// DECODED KINDS (File, Upload), whose input is an encoded file that the backend decodes on the device into the slot's device input,
// key.in_bytes() per job, in place of h2d:
//   std::shared_ptr<void> file_plan(const uint8_t* file, size_t bytes, int* h, int* w, size_t* room);
//                                                              submitting thread, no lock: reads the file's head and checks all of it;
//                                                              throws Error when the file is refused.  *room: bytes file_stage needs at most
//   std::shared_ptr<void> upload_plan(const uint8_t* file, size_t bytes, int max_dim, int* h, int* w, size_t* room, int up[4]);
//                                                              file_plan for an upload: *h, *w = the FITTED size, up = the rest of its key
//   size_t file_stage(void* head, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room);
//                                                              submitting thread, no lock: what the device needs of the file into dst (the
//                                                              job's place in pin_in, or the job's own vector); -> bytes written; throws Error
//   void decode(SlotBufs&, int first, int count, const SlotKey&, void* const* heads, const size_t* used);
//                                                              launcher, in place of h2d, WITHOUT the batcher's lock, copy-in stream: jobs first ..
//                                                              first + count - 1 of the slot, their staged bytes at pin_in + key.in_bytes() * index;
//                                                              an Upload's files decoded at their stored size, oriented and fitted; throws Error
//   int file_status(SlotBufs&, int index);                     after wait_done: 0, or what the device found wrong with that job's data

// the room rule of upload jobs (submit_upload; ire_upload_plan says the same of the same file)
constexpr const char* kUploadRoomReason = "invalid: the file's entropy-coded data may be larger than its fitted pixels (decode it with the host codec)";
constexpr int kPollTooSmall = -2;     // Batcher::poll: the caller's buffer is shorter than the result; the job stays pending

template <class Backend>
class Batcher {
  public:
    using clk = std::chrono::steady_clock;
    explicit Batcher(Backend& be) : be_(be) { const char* t = std::getenv("IRE_BATCH_TRACE"); trace_ = t && t[0] == '1'; }
    Batcher(const Batcher&) = delete;
    Batcher& operator=(const Batcher&) = delete;

    ~Batcher() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        qcv_.notify_all();
        if (launcher_.joinable()) launcher_.join();      // launches what is still gathered (and staged), then exits
        ccv_.notify_all();
        if (completer_.joinable()) completer_.join();    // completes every batch in flight
        be_.drain();
        for (auto& S : slots_) { be_.release(S.b); S = BatchSlot{}; }
    }

    // One timed wait for every caller.  The product waits on the steady clock (pthread_cond_clockwait).  The ThreadSanitizer
    // build of tests/native defines IRE_BATCHER_SYSCLOCK_WAITS: gcc 11's libtsan does not intercept pthread_cond_clockwait, so it
    // misses the unlock / relock inside the wait and reports every other thread's critical section as a race; the same deadline
    // on the system clock goes through pthread_cond_timedwait, which it does intercept.  Returns false at the deadline.
    template <class Lock>
    static bool wait_deadline(std::condition_variable& cv, Lock& lk, clk::time_point tp) {
#ifdef IRE_BATCHER_SYSCLOCK_WAITS
        const auto left = tp - clk::now();
        if (left <= clk::duration::zero()) return false;
        return cv.wait_until(lk, std::chrono::system_clock::now() + left) == std::cv_status::no_timeout;
#else
        return cv.wait_until(lk, tp) == std::cv_status::no_timeout;
#endif
    }

    // Queue one image.  Throws Error (invalid size is the caller's check); the returned job is pending.
    std::shared_ptr<Job> submit(const uint8_t* rgb, int h, int w, int is_jpeg, const double* scores) {
        auto j = std::make_shared<Job>();
        j->key.h = h; j->key.w = w;
        set_image(*j, 0, is_jpeg != 0, scores);
        // the ONE host copy of the input: caller's buffer -> pinned slot, in the caller's thread
        stage(j, j->key.in_bytes(), [&](uint8_t* dst) { std::memcpy(dst, rgb, j->key.in_bytes()); return j->key.in_bytes(); });
        return j;
    }

    // Queue one encoded file (is_jpeg: what the ABI entry found it to be; the backend's hooks dispatch on the head they made).
    // The head is parsed and the scan is cut HERE, in the submitting thread, straight into the job's place in
    // the slot's pinned input; the launcher only hands the staged jobs to the backend's decode.  Throws Error when the backend refuses
    // the file: no job exists then.
    std::shared_ptr<Job> submit_file(const uint8_t* file, size_t bytes, const double* scores, bool is_jpeg = true) {
        auto j = std::make_shared<Job>();
        size_t room = 0;
        j->key.kind = JobKind::File;
        j->file = be_.file_plan(file, bytes, &j->key.h, &j->key.w, &room);
        if (room > j->key.in_bytes()) fail(IRE_ERR_INVALID_INPUT, "invalid: the file's entropy-coded data may be larger than its pixels (it stays with the host codec)");
        set_image(*j, 0, is_jpeg, scores);
        stage(j, room, [&](uint8_t* dst) { return be_.file_stage(j->file.get(), file, bytes, dst, room); });
        return j;
    }

    // Queue one encoded upload: a file job that the backend orients by the file's EXIF tag and fits inside max_dim on the device, after
    // the decode and before the network.  The job's h, w are the fitted size; its place in the slot's input holds that many pixels, and a
    // file whose cut scan may need more is refused: no job exists then.
    std::shared_ptr<Job> submit_upload(const uint8_t* file, size_t bytes, int max_dim, const double* scores, bool is_jpeg = true) {
        auto j = std::make_shared<Job>();
        size_t room = 0;
        j->key.kind = JobKind::Upload;
        j->file = be_.upload_plan(file, bytes, max_dim, &j->key.h, &j->key.w, &room, j->key.up);
        if (room > j->key.in_bytes()) fail(IRE_ERR_INVALID_INPUT, kUploadRoomReason);
        set_image(*j, 0, is_jpeg, scores);
        stage(j, room, [&](uint8_t* dst) { return be_.file_stage(j->file.get(), file, bytes, dst, room); });
        return j;
    }

    // Queue one fusion job: k = 2..3 views of h x w.  All k views are staged HERE, in the submitting thread: one copy each into the
    // job's k consecutive places of the pinned slot (or into the job's own vector on the overflow path).  is_jpeg / has_scores: [k] or
    // null (all JPEG / none supplied); scores: [k][7], read where has_scores says so.
    std::shared_ptr<Job> submit_group(const uint8_t* const* views, int k, int h, int w, const uint8_t* is_jpeg, const uint8_t* has_scores, const double* scores) {
        if (k < 2 || k > 3) fail(IRE_ERR_INVALID_INPUT, "invalid view count for fusion: expected 2..3");
        if (be_.max_batch() < k) fail(IRE_ERR_INVALID_INPUT, "invalid view count for fusion: the engine's max_batch is smaller than the number of views");
        auto j = std::make_shared<Job>();
        j->key.h = h; j->key.w = w; j->key.kind = JobKind::Group; j->key.k = k;
        for (int v = 0; v < k; ++v) set_image(*j, v, !is_jpeg || is_jpeg[v], has_scores && has_scores[v] ? scores + 7 * v : nullptr);
        const size_t ib = j->key.image_bytes();
        stage(j, j->key.in_bytes(), [&](uint8_t* dst) {
            for (int v = 0; v < k; ++v) std::memcpy(dst + ib * v, views[v], ib);       // the ONE host copy of each view, in the caller's thread
            return j->key.in_bytes();
        });
        return j;
    }

    // Wait up to timeout_ms (< 0: forever).  Returns IRE_OK (outputs filled, job finished), IRE_ERR_TIMEOUT (job still pending:
    // poll again or release) or the job's failure status (*err_out = its message; job finished).
    int poll(const std::shared_ptr<Job>& j, int timeout_ms, uint8_t* out_rgb, double* scores_out, ire_timings* t, std::string* err_out) {
        return poll(j, timeout_ms, out_rgb, (size_t)-1, nullptr, scores_out, t, err_out);
    }

    // The same with the size of the caller's buffer and the result's real length (*len_out, may be null).  A result longer than cap
    // is not copied: kPollTooSmall, *len_out says what is needed, the job stays pending (nothing is lost to a short buffer).
    int poll(const std::shared_ptr<Job>& j, int timeout_ms, uint8_t* out_rgb, size_t cap, size_t* len_out, double* scores_out, ire_timings* t, std::string* err_out) {
        BatchSlot* S = nullptr;
        {
            std::unique_lock<std::mutex> lk(mu_);
            auto done = [&] { return j->status >= 0; };
            if (timeout_ms < 0) dcv_.wait(lk, done);
            else {
                const auto until = clk::now() + std::chrono::milliseconds(timeout_ms);
                while (!done()) if (!wait_deadline(dcv_, lk, until) && !done()) return IRE_ERR_TIMEOUT;
            }
            S = j->slot;
            if (S) S->reading += 1;        // the slot cannot be recycled (or evicted) while this thread copies from it
        }
        const int st = j->status;
        if (st == IRE_OK) {
            const size_t ob = be_.out_bytes(j->key.h, j->key.w);
            size_t len = ob;
            const uint8_t* src = be_.result_view(S ? S->b.pin_out + ob * j->idx : j->out.data(), j->key.h, j->key.w, &len);
            if (len_out) *len_out = len;
            if (len > cap) {
                if (S) { std::lock_guard<std::mutex> lk(mu_); S->reading -= 1; qcv_.notify_all(); }
                return kPollTooSmall;
            }
            // the ONE host copy of the output: pinned slot -> caller's buffer, in the caller's thread; only the real length moves
            if (out_rgb) std::memcpy(out_rgb, src, len);
            if (scores_out) std::memcpy(scores_out, j->scores, sizeof(double) * 7);
            if (t) *t = j->t;
        } else if (err_out) *err_out = j->err;
        if (S) {
            std::lock_guard<std::mutex> lk(mu_);
            S->reading -= 1;
            drop_reader(*S, *j);
        }
        return st;
    }

    // Give up a job without fetching it (a rejected promise, a timed-out poll the caller will not repeat): frees what only this
    // handle kept alive -- its place among the slot's unread results, its overflow pixels.
    void release(const std::shared_ptr<Job>& j) {
        std::lock_guard<std::mutex> lk(mu_);
        if (j->status >= 0) {                     // complete: nobody will read it
            if (j->slot) drop_reader(*j->slot, *j);
            j->out.clear(); j->out.shrink_to_fit();
            return;
        }
        for (auto it = overflow_.begin(); it != overflow_.end(); ++it)
            if (it->get() == j.get()) { overflow_.erase(it); j->status = IRE_ERR_INTERNAL; j->in.clear(); j->in.shrink_to_fit(); return; }
        cnt_.abandoned += 1;
        j->abandoned = true;                      // gathered or in flight: the batch runs as staged, its completion skips this job
    }

    // how often the rare paths ran (tests assert that they did)
    struct Counters { long batches = 0, overflowed = 0, evicted = 0, abandoned = 0, failed_batches = 0; };
    Counters counters() { std::lock_guard<std::mutex> lk(mu_); return cnt_; }

    // no job queued, in flight or delivered but not yet polled: every slot is FREE and nothing overflows
    bool idle() {
        std::lock_guard<std::mutex> lk(mu_);
        if (!overflow_.empty()) return false;
        for (const BatchSlot& S : slots_) if (S.state != BatchSlot::FREE) return false;
        return true;
    }

    int queue_depth() {
        std::lock_guard<std::mutex> lk(mu_);
        int depth = (int)overflow_.size();
        for (int si : open_order_) depth += (int)slots_[si].jobs.size();
        return depth;
    }

  private:
    // (mu_ held) at the top of every submit: refuses while shutting down; the first one starts the backend and the service threads
    void start_locked(const SlotKey& key) {
        if (stop_) fail(IRE_ERR_UNAVAILABLE, "service unavailable: the engine is shutting down");
        if (started_) return;
        be_.start();
        // staging for the three slots of a steady stream now, at this first shape (pinning 3 x 2 x max_batch images takes tens
        // of ms): the first job pays it once, instead of later jobs paying it one slot at a time in the middle of a stream
        for (int i = 0; i < kSlotsEager; ++i) be_.reserve(slots_[i].b, staging_bytes(key), be_.max_batch());
        launcher_ = std::thread([this] { launcher_loop(); });
        completer_ = std::thread([this] { completer_loop(); });
        started_ = true;
    }

    // a slot's staging per direction: max_batch images of the key's size, or as many results
    size_t staging_bytes(const SlotKey& key) const { return std::max(key.image_bytes(), be_.out_bytes(key.h, key.w)) * (size_t)be_.max_batch(); }

    // image v of a job: its is_jpeg flag and, where the caller supplied them, its scores
    static void set_image(Job& j, int v, bool is_jpeg, const double* scores) {
        j.v_jpeg[v] = is_jpeg ? 1 : 0;
        if (scores) { std::memcpy(j.v_scores[v], scores, sizeof(double) * 7); j.v_has[v] = 1; }
    }

    // The ONE staging path of every submit: a place for job j (whose key and per-image flags are set) -- the next index of a slot of its
    // key, or, when every slot is busy or jobs are already overflowing (they keep their order), `room` bytes of its own that the
    // launcher copies into a slot later -- then write(dst) -> bytes written puts the input there, in the caller's thread, without the
    // lock.  `room`: what write needs at most (key.in_bytes(), or less for a file's scan).
    //  * A throw before the job has its place (shutting down, no staging memory) reaches the submitter: no job exists.
    //  * A throw from write comes after it -- the slot already counts on the job becoming staged -- so it is recorded: the job is staged
    //    with nothing to decode (file_used = 0) and fails alone, with that status and reason, when its batch completes.  Only the decoded
    //    kinds' writers can throw (file_plan checked the whole file, so file_stage cannot refuse it unless the caller changed the bytes
    //    meanwhile; or a bad_alloc); the others are memcpys.
    //  * On the overflow path the bytes stay in j->in, trimmed to what was written.
    template <class Write>
    void stage(const std::shared_ptr<Job>& j, size_t room, Write&& write) {
        uint8_t* dst = nullptr;
        {
            std::lock_guard<std::mutex> lk(mu_);
            start_locked(j->key);
            const int si = overflow_.empty() ? slot_for(j->key) : -1;
            if (si >= 0) { slot_add(si, j); dst = slots_[si].b.pin_in + j->key.in_bytes() * j->idx; }
        }
        const bool in_slot = dst != nullptr;
        if (!in_slot) { j->in.resize(room); dst = j->in.data(); }
        size_t used = 0;
        int code = IRE_OK;
        std::string why;
        try { used = write(dst); }
        catch (const Error& e) { code = e.code; why = e.msg; used = 0; }
        catch (const std::exception& e) { code = IRE_ERR_UNAVAILABLE; why = std::string("service unavailable: ") + e.what(); used = 0; }
        {
            std::lock_guard<std::mutex> lk(mu_);
            j->file_used = used;
            if (code != IRE_OK) { j->stage_status = code; j->err = why; }
            if (!in_slot) { j->in.resize(used); overflow_.push_back(j); cnt_.overflowed += 1; }
            j->staged = true;
        }
        qcv_.notify_all();
    }

    // (mu_ held) a job's result has been fetched or given up: the slot is free once the last one has
    void drop_reader(BatchSlot& S, Job& j) {
        j.slot = nullptr;
        S.unread -= 1;
        if (S.unread == 0 && S.state == BatchSlot::DONE) { S.jobs.clear(); S.state = BatchSlot::FREE; }
        qcv_.notify_all();                        // a FREE (or now evictable) slot: overflow jobs may be waiting for it
    }

    // (mu_ held) an OPEN slot of this key with room, else a FREE one opened for it, else -1.  May allocate staging (first use
    // of a shape: once).  A DONE slot nobody is reading is evicted when nothing else is left: its unfetched outputs move to
    // their jobs' own vectors (the extra copy only a caller that lets a slot's worth of batches pile up unpolled ever pays).
    int slot_for(const SlotKey& key) {
        for (auto it = open_order_.rbegin(); it != open_order_.rend(); ++it) {
            BatchSlot& S = slots_[*it];
            if (S.key == key && (int)S.jobs.size() < capacity(S)) return *it;
        }
        int pick = -1;
        const size_t need = staging_bytes(key);
        for (int i = 0; i < kSlots && pick < 0; ++i) if (slots_[i].state == BatchSlot::FREE && slots_[i].b.cap >= need) pick = i;     // one whose staging exists
        for (int i = 0; i < kSlots && pick < 0; ++i) if (slots_[i].state == BatchSlot::FREE) pick = i;
        for (int i = 0; i < kSlots && pick < 0; ++i) {
            BatchSlot& S = slots_[i];
            if (S.state != BatchSlot::DONE || S.reading) continue;
            const size_t ib = be_.out_bytes(S.key.h, S.key.w);
            // job by job, each move complete before the slot forgets the job: a bad_alloc half way leaves a consistent DONE slot
            for (auto& j : S.jobs)
                if (j->slot == &S) {
                    j->out.assign(S.b.pin_out + ib * j->idx, S.b.pin_out + ib * (j->idx + 1));
                    j->slot = nullptr;
                    S.unread -= 1;
                    cnt_.evicted += 1;
                }
            S.jobs.clear(); S.unread = 0; S.state = BatchSlot::FREE;
            pick = i;
        }
        if (pick < 0) return -1;
        BatchSlot& S = slots_[pick];
        be_.reserve(S.b, need, be_.max_batch());  // strong guarantee: a throw leaves the slot FREE with what it had
        S.state = BatchSlot::OPEN; S.key = key; S.jobs.clear(); S.h2d_issued = 0; S.unread = S.reading = 0;
        S.status = IRE_OK; S.err.clear();
        S.first_arrival = S.last_arrival = clk::now();
        open_order_.push_back(pick);
        return pick;
    }

    // jobs a slot holds: max_batch images, so max_batch / k fusion jobs of k views, and never more than one fused launch takes
    int capacity(const BatchSlot& S) const { return S.key.k ? std::min(be_.max_batch() / S.key.k, kGroupMaxJobs) : be_.max_batch(); }

    // (mu_ held) reserve the next index of slot si for job j
    void slot_add(int si, const std::shared_ptr<Job>& j) {
        BatchSlot& S = slots_[si];
        j->slot = &S; j->idx = (int)S.jobs.size();
        const int per = S.key.images_per_job();    // images of the job: they take places idx * per .. of the slot
        for (int v = 0; v < per; ++v) {
            const int at = j->idx * per + v;
            S.b.pin_jp[at] = j->v_jpeg[v];
            S.has_sc[at] = j->v_has[v];
            if (j->v_has[v]) std::memcpy(S.b.pin_sc_in + 7 * at, j->v_scores[v], sizeof(double) * 7);
        }
        S.jobs.push_back(j);
        S.last_arrival = clk::now();
        if (j->idx == 0) S.first_arrival = S.last_arrival;
    }

    // (launcher, mu_ held) H2D of every image staged so far, in index order, on the copy-in stream: rides under the previous
    // batch's compute.  A failure is recorded in the slot (the launch then fails the batch).
    // File jobs go to the backend's decode instead, and only once the batch is full or closing: a decode costs a fixed set of
    // launches whatever the number of images (measured, profiles/jpeg_file_jobs.md: one 1024^2 file 2.5 ms, eight 4.7 ms), so pushing
    // them one by one as they arrive would cap the slot at the one-file rate.  A full batch still goes at once and its decode runs on
    // the copy-in stream under the previous batch's compute.  The decode is called with mu_ RELEASED (it packs records, may wait for
    // an upload and enqueues a dozen operations; submitters and pollers must not queue behind that): the slot is full or CLOSED, so
    // nobody adds to it meanwhile, and only this thread moves a slot out of OPEN / CLOSED.
    void slot_push_h2d(BatchSlot& S, std::unique_lock<std::mutex>& lk, bool closing) {
        int upto = S.h2d_issued;
        while (upto < (int)S.jobs.size() && S.jobs[upto]->staged) ++upto;
        if (upto == S.h2d_issued || S.status != IRE_OK) return;
        if (S.key.decoded() && !closing && upto < be_.max_batch()) return;
        int code = IRE_OK;
        std::string why;
        try {
            if (S.key.decoded()) push_decode(S, upto, lk);
            else be_.h2d(S.b, S.key.in_bytes() * S.h2d_issued, S.key.in_bytes() * (size_t)(upto - S.h2d_issued));
        } catch (const Error& e) { code = e.code; why = e.msg; }
        catch (const std::exception& e) { code = IRE_ERR_UNAVAILABLE; why = std::string("service unavailable: ") + e.what(); }      // (a decode's host allocations)
        if (!lk.owns_lock()) lk.lock();
        if (code != IRE_OK) { S.status = code; S.err = why; }
        S.h2d_issued = upto;
    }

    // (launcher) jobs h2d_issued .. upto - 1 of a slot of a decoded kind to the backend's decode; collects under mu_, calls without it
    void push_decode(BatchSlot& S, int upto, std::unique_lock<std::mutex>& lk) {
        void* heads[kMaxBatch];
        size_t used[kMaxBatch];
        const int first = S.h2d_issued, count = upto - first;
        for (int i = 0; i < count; ++i) { heads[i] = S.jobs[first + i]->file.get(); used[i] = S.jobs[first + i]->file_used; }
        const SlotKey key = S.key;
        lk.unlock();
        be_.decode(S.b, first, count, key, heads, used);
        lk.lock();
    }

    // (mu_ held) what fails job i of a completed batch ALONE: its staging failed at submit, or the device flagged its data
    bool job_failed_alone(BatchSlot& S, int i, Job& j) {
        if (j.stage_status != IRE_OK) { j.status = j.stage_status; return true; }       // (j.err holds the reason since submit)
        if (!S.key.decoded()) return false;
        const int st = be_.file_status(S.b, i);
        if (st != 0) {        // (is_jpeg = false on a decoded kind: the ABI entry found a PNG)
            j.status = IRE_ERR_INVALID_INPUT;
            j.err = std::string("invalid: corrupt ") + (j.v_jpeg[0] ? "JPEG" : "PNG") + " data (decoder status " + std::to_string(st) + ")";
            return true;
        }
        return false;
    }

    void complete_jobs(BatchSlot& S, const ire_timings& t) {     // mu_ held
        const int n = (int)S.jobs.size();
        int readers = 0;
        for (int i = 0; i < n; ++i) {
            Job& j = *S.jobs[i];
            if (S.status == IRE_OK && !j.abandoned && job_failed_alone(S, i, j)) { j.slot = nullptr; continue; }
            if (S.status == IRE_OK && !j.abandoned) { std::memcpy(j.scores, S.b.pin_sc + 7 * i, sizeof(double) * 7); j.t = t; ++readers; }
            else j.slot = nullptr;
            j.err = S.err;
            j.status = j.abandoned && S.status == IRE_OK ? IRE_ERR_INTERNAL : S.status;
        }
        if (S.status == IRE_OK && readers > 0) { S.state = BatchSlot::DONE; S.unread = readers; }
        else { S.jobs.clear(); S.state = BatchSlot::FREE; }
    }

    static void fail_job(Job& j, int code, const std::string& msg) { j.status = code; j.err = msg; j.in.clear(); j.in.shrink_to_fit(); }

    void launcher_loop() {
        be_.thread_enter("launcher");
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            // jobs that found no free slot at submit time: stage them now (this thread copies), oldest first
            while (!overflow_.empty()) {
                std::shared_ptr<Job> j = overflow_.front();
                int si = -1;
                try { si = slot_for(j->key); }
                catch (const Error& e) { fail_job(*j, e.code, e.msg); overflow_.pop_front(); dcv_.notify_all(); continue; }
                catch (const std::exception& e) {      // bad_alloc while evicting a DONE slot: this job fails, the service thread lives
                    fail_job(*j, IRE_ERR_UNAVAILABLE, std::string("service unavailable: ") + e.what()); overflow_.pop_front(); dcv_.notify_all(); continue;
                }
                if (si < 0) break;
                overflow_.pop_front();
                slot_add(si, j);
                BatchSlot& S = slots_[si];
                if (!j->in.empty()) std::memcpy(S.b.pin_in + S.key.in_bytes() * j->idx, j->in.data(), j->in.size());
                j->in.clear(); j->in.shrink_to_fit();
            }
            if (open_order_.empty()) {
                if (stop_ && overflow_.empty()) break;
                // nothing gathered: a submit wakes this thread; overflow jobs wait for a slot, and everything that frees one or makes
                // one evictable (poll, release, the completer) notifies qcv_
                qcv_.wait(lk);
                continue;
            }
            const int si = open_order_.front();
            BatchSlot& S = slots_[si];
            slot_push_h2d(S, lk, false);
            const bool full = (int)S.jobs.size() >= capacity(S);
            if (!full && !stop_ && S.status == IRE_OK && open_order_.size() == 1) {
                bool gpu_busy = false;
                if (last_launched_ >= 0) {
                    BatchSlot& P = slots_[last_launched_];
                    gpu_busy = P.state == BatchSlot::INFLIGHT && be_.computing(P.b);
                }
                // the completer notifies when that batch's compute ends (the bound only covers a lost wake-up)
                if (gpu_busy) { (void)wait_deadline(qcv_, lk, clk::now() + std::chrono::milliseconds(2)); continue; }
                const auto now = clk::now();
                const auto go = std::min(S.last_arrival + std::chrono::microseconds(kLingerQuietUs), S.first_arrival + std::chrono::microseconds(kLingerMaxUs));
                if (now < go) { (void)wait_deadline(qcv_, lk, go); continue; }     // an arrival re-evaluates; otherwise one wake-up at the deadline
            }
            if (trace_) {
                const auto now = clk::now();
                std::fprintf(stderr, "[batch] slot %d n %d full %d quiet_us %lld age_us %lld since_prev_launch_us %lld open %zu inflight %zu\n", si, (int)S.jobs.size(), (int)full,
                             (long long)std::chrono::duration_cast<std::chrono::microseconds>(now - S.last_arrival).count(),
                             (long long)std::chrono::duration_cast<std::chrono::microseconds>(now - S.first_arrival).count(),
                             (long long)std::chrono::duration_cast<std::chrono::microseconds>(now - last_launch_time_).count(), open_order_.size(), inflight_.size());
                last_launch_time_ = now;
            }
            // launch: no more reservations, wait for the copies still running in submitting threads
            S.state = BatchSlot::CLOSED;
            open_order_.pop_front();
            qcv_.wait(lk, [&] { for (auto& j : S.jobs) if (!j->staged) return false; return true; });
            slot_push_h2d(S, lk, true);
            const int n = (int)S.jobs.size();
            bool wanted = false;
            for (auto& j : S.jobs) wanted = wanted || !j->abandoned;
            if (!wanted && S.status == IRE_OK) {       // every job of the batch was given up while it gathered: nothing to compute
                complete_jobs(S, ire_timings{});
                continue;
            }
            lk.unlock();
            try {
                if (S.status != IRE_OK) throw Error{S.status, S.err};
                be_.launch(S.b, n, S.key, S.has_sc);       // (no lock: the slot is CLOSED, only this thread touches its key)
            } catch (const Error& e) { S.status = e.code; S.err = e.msg; }
            catch (const std::exception& e) { S.status = IRE_ERR_INTERNAL; S.err = std::string("internal: ") + e.what(); }
            if (S.status != IRE_OK) be_.drain();   // whatever was enqueued before the failure may still touch the slot's buffers
            lk.lock();
            cnt_.batches += 1;
            if (S.status != IRE_OK) cnt_.failed_batches += 1;
            if (S.status == IRE_OK) {
                S.state = BatchSlot::INFLIGHT;
                inflight_.push_back(si);
                last_launched_ = si;
                ccv_.notify_all();
            } else {
                complete_jobs(S, ire_timings{});
                dcv_.notify_all();
            }
        }
        launcher_done_ = true;
        ccv_.notify_all();
    }

    void completer_loop() {
        be_.thread_enter("completer");
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            ccv_.wait(lk, [&] { return !inflight_.empty() || launcher_done_; });
            if (inflight_.empty()) break;
            BatchSlot& S = slots_[inflight_.front()];
            lk.unlock();
            be_.wait_compute(S.b);
            { std::lock_guard<std::mutex> g(mu_); }   // (the launcher is either before its check of computing() or already waiting: no lost wake-up)
            qcv_.notify_all();                     // the GPU is free: a batch that kept gathering behind this one may go
            ire_timings t{};
            int st = IRE_OK; std::string err;
            try { be_.wait_done(S.b, t); }
            catch (const Error& e) { st = e.code; err = e.msg; }
            lk.lock();
            if (st != IRE_OK) { S.status = st; S.err = err; }
            inflight_.pop_front();
            complete_jobs(S, t);
            dcv_.notify_all();
            qcv_.notify_all();
        }
    }

    Backend& be_;
    std::mutex mu_;
    std::condition_variable qcv_, dcv_, ccv_;      // launcher wake-ups | job completion | completer wake-ups
    BatchSlot slots_[kSlots];
    std::deque<int> open_order_;                   // OPEN slots, oldest first
    std::deque<int> inflight_;                     // INFLIGHT slots, launch order
    std::deque<std::shared_ptr<Job>> overflow_;    // submitted while no slot was free: staged by the launcher later
    int last_launched_ = -1;
    Counters cnt_;
    bool trace_ = false;                           // IRE_BATCH_TRACE=1: one stderr line per launched batch (why it went, how long it gathered)
    clk::time_point last_launch_time_ = clk::now();
    std::thread launcher_, completer_;
    bool stop_ = false, launcher_done_ = false, started_ = false;
};

}  // namespace ire
