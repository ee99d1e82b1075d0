// lane_pump.hpp — the body of a copier thread: jobs from an owner onto copy lanes in rotation (the read-out ring, the peer copier and
// the shared-memory ring's publisher, capi_readout.hip and shm_ring.inc). Host only and without a HIP or HSA include, so that
// tests/lane_pump_check.cpp runs it alone, against lanes that land when the test says so, under the thread and address sanitizers.
//
// `lanes`: finish(lane) waits for the lane's copy and says whether it succeeded; landed(lane) asks without waiting.
// `owner`: its queue, its locks and what a finished copy means to it —
//     bool take(Job&, bool sleep)      the next job; false: none queued — when `sleep`, only once the owner is stopped as well
//     bool ready(const Job&)           waits until the job's source is complete; false: it never will be
//     LaneIssue issue(int, const Job&) puts the copy on the lane
//     void landed(const Job&, bool ok) the job's copy has ended: what lies at its destination is the frame, or (`ok` false) is not
//     bool failed(const Job&)          the job was not ready or not issued: true to go on with the next one, false to end the thread
#pragma once

enum class LaneIssue { issued, failed, skipped };                   // skipped: the owner has accounted for the job itself, the lane stays free

// `report_early`: lanes that have landed are reported at once, in any order, not when their turn comes round (a continuously fed queue
// never runs empty, and the thread is about to block on the NEXT job's source). Only for owners whose landed() may be told out of order.
template <class Job, class Lanes, class Owner> void lane_pump(Lanes& lanes, int lane_count, bool report_early, Owner& owner) {
    constexpr int MOST = 4;
    Job in_lane[MOST];
    bool held[MOST] = {};
    int next = 0;
    auto finish = [&](int lane) {
        if (!held[lane]) return;
        const bool ok = lanes.finish(lane);
        held[lane] = false;
        owner.landed(in_lane[lane], ok);
    };
    auto report_landed = [&] { if (report_early) for (int lane = 0; lane < lane_count; lane++) if (held[lane] && lanes.landed(lane)) finish(lane); };
    for (;;) {
        Job job;
        if (!owner.take(job, false)) {                               // nothing to issue: let what is in flight land (in issue order), then sleep
            for (int k = 0; k < lane_count; k++) finish((next + k) % lane_count);
            if (!owner.take(job, true)) return;
        }
        report_landed();
        const bool ready = owner.ready(job);
        report_landed();
        finish(next);                                                // the lane's previous copy
        const LaneIssue answer = ready ? owner.issue(next, job) : LaneIssue::failed;
        if (answer == LaneIssue::failed && !owner.failed(job)) return;
        if (answer != LaneIssue::issued) continue;
        in_lane[next] = job;
        held[next] = true;
        next = (next + 1) % lane_count;
    }
}
