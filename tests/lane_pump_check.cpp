// The copier loop of the read-out (shaderflow_amd/csrc/lane_pump.hpp), alone: a program of its own, built with the thread sanitizer and
// with the address and undefined-behaviour sanitizers by tests/test_host_lane_pump.py. The lanes are a fake whose copies land when the
// test says so, the owner is a plain queue of job numbers. Every case runs under a watchdog: one that has not finished after 20 s
// prints its name and aborts. Nothing here sleeps to find out whether something happened — a case waits for the state it needs.
#include "lane_pump.hpp"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#define CHECK(condition) do { if (!(condition)) { fprintf(stderr, "%s:%d: case '%s': %s does not hold\n", __FILE__, __LINE__, g_case, #condition); abort(); } } while (0)
static const char* g_case = "";

// everything the pump's thread, the case's thread and the helpers share lives behind ONE mutex and ONE condition variable
struct Rig {
    std::mutex mutex;
    std::condition_variable moved;
    // the lanes
    int lane_count;
    int in_lane[4] = {-1, -1, -1, -1};              // the job whose copy is in the lane and has not been finished
    std::vector<char> may_land, bad;                // per job: its copy may end; it ends as a failure
    std::vector<int> issued, issue_lane;            // jobs in issue order, and the lane each went to
    int refuse = -1;                                // issue() of this job fails
    // the owner
    std::deque<int> queue;
    bool stop = false, sleeping = false, go_on = true;
    int unready = -1, skip = -1, gate = -1, in_ready = -1;   // gate: ready() of this job blocks until `gate_open`
    bool gate_open = false;
    std::vector<std::pair<int, bool>> reports;
    std::vector<int> failures;

    Rig(int lanes, int jobs) : lane_count(lanes), may_land(jobs, 0), bad(jobs, 0) {}

    // the lanes the pump sees: finish() blocks until the case lets the copy land
    struct Lanes {
        Rig& rig;
        bool issue(int lane, int job) { return rig.lane_issue(lane, job); }
        bool landed(int lane) { return rig.lane_landed(lane); }
        bool finish(int lane) { return rig.lane_finish(lane); }
    };
    // the owner the pump sees: a plain queue
    struct Owner {
        Rig& rig;
        Lanes& lanes;
        bool take(int& job, bool sleep) { return rig.take(job, sleep); }
        bool ready(int job) { return rig.ready(job); }
        LaneIssue issue(int lane, int job) { return rig.skips(job) ? LaneIssue::skipped : lanes.issue(lane, job) ? LaneIssue::issued : LaneIssue::failed; }
        void landed(int job, bool ok) { rig.report(job, ok); }
        bool failed(int job) { return rig.failed(job); }
    };

    bool lane_issue(int lane, int job) {
        std::lock_guard<std::mutex> lock(mutex);
        CHECK(lane >= 0 && lane < lane_count);
        CHECK(in_lane[lane] < 0);                   // never onto a lane whose copy has not been finished
        if (job == refuse) return false;
        in_lane[lane] = job; issued.push_back(job); issue_lane.push_back(lane);
        moved.notify_all();
        return true;
    }
    bool lane_landed(int lane) {
        std::lock_guard<std::mutex> lock(mutex);
        return in_lane[lane] < 0 || may_land[in_lane[lane]];
    }
    bool lane_finish(int lane) {
        std::unique_lock<std::mutex> lock(mutex);
        if (in_lane[lane] < 0) return true;
        const int job = in_lane[lane];
        moved.wait(lock, [&] { return may_land[job] != 0; });
        in_lane[lane] = -1;
        return !bad[job];
    }
    bool take(int& job, bool sleep) {
        std::unique_lock<std::mutex> lock(mutex);
        if (sleep) { sleeping = true; moved.notify_all(); moved.wait(lock, [&] { return stop || !queue.empty(); }); sleeping = false; }
        if (queue.empty()) return false;
        job = queue.front(); queue.pop_front();
        return true;
    }
    bool ready(int job) {
        std::unique_lock<std::mutex> lock(mutex);
        in_ready = job; moved.notify_all();
        if (job == gate) moved.wait(lock, [&] { return gate_open; });
        in_ready = -1;
        return job != unready;
    }
    bool skips(int job) { std::lock_guard<std::mutex> lock(mutex); return job == skip; }
    void report(int job, bool ok) {
        std::lock_guard<std::mutex> lock(mutex);
        CHECK(may_land[job]);                       // never before its copy was allowed to land
        for (int lane = 0; lane < 4; lane++) CHECK(in_lane[lane] != job);
        reports.push_back({job, ok});
        moved.notify_all();
    }
    bool failed(int job) {
        std::lock_guard<std::mutex> lock(mutex);
        failures.push_back(job);
        moved.notify_all();
        return go_on;
    }

    // the case's side
    void push(int first, int count) { std::lock_guard<std::mutex> lock(mutex); for (int k = 0; k < count; k++) queue.push_back(first + k); moved.notify_all(); }
    void land(int job) { std::lock_guard<std::mutex> lock(mutex); may_land[job] = 1; moved.notify_all(); }
    void halt() { std::lock_guard<std::mutex> lock(mutex); stop = true; moved.notify_all(); }
    template <class F> void await(F state) { std::unique_lock<std::mutex> lock(mutex); moved.wait(lock, state); }
    // lets the copies land in issue order, as they are issued, until `count` have
    void land_in_order(int count) {
        for (int k = 0; k < count; k++) {
            int job = -1;
            await([&] { if ((int)issued.size() > k) job = issued[k]; return job >= 0; });
            land(job);
        }
    }
    std::thread start(bool report_early) { return std::thread([this, report_early] { Lanes lanes{*this}; Owner owner{*this, lanes}; lane_pump<int>(lanes, lane_count, report_early, owner); }); }
    // what holds at the end of every case: the k-th copy issued went to lane k modulo the lane count; nobody was reported twice
    void check_rotation() {
        for (size_t k = 0; k < issued.size(); k++) CHECK(issue_lane[k] == (int)(k % lane_count));
        std::vector<int> seen;
        for (auto& report : reports) seen.push_back(report.first);
        std::sort(seen.begin(), seen.end());
        CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end());
    }
    bool reported_in_order(const std::vector<int>& jobs) {
        if (reports.size() != jobs.size()) return false;
        for (size_t k = 0; k < jobs.size(); k++) if (reports[k].first != jobs[k]) return false;
        return true;
    }
};

static std::vector<int> range(int from, int to, int without = -1) {
    std::vector<int> jobs;
    for (int k = from; k < to; k++) if (k != without) jobs.push_back(k);
    return jobs;
}

static void run(const char* name, const std::function<void()>& body) {
    g_case = name;
    std::mutex mutex; std::condition_variable over; bool done = false;
    std::thread watchdog([&] {
        std::unique_lock<std::mutex> lock(mutex);
        // (the system clock: a wait on the steady one goes through pthread_cond_clockwait, which older thread sanitizers do not know)
        if (!over.wait_until(lock, std::chrono::system_clock::now() + std::chrono::seconds(20), [&] { return done; })) { fprintf(stderr, "case '%s' has not finished after 20 s\n", name); abort(); }
    });
    body();
    { std::lock_guard<std::mutex> lock(mutex); done = true; }
    over.notify_all();
    watchdog.join();
    printf("ok %s\n", name);
}

// 13 jobs over 1, 2 and 4 lanes, both modes: every job reported once, in order when the copies land in order
static void turns(int lanes, bool early) {
    Rig rig(lanes, 13);
    std::thread pump = rig.start(early);
    rig.push(0, 5);
    rig.land_in_order(5);
    rig.await([&] { return rig.reports.size() == 5; });
    rig.push(5, 8);
    rig.land_in_order(13);
    rig.await([&] { return rig.reports.size() == 13; });
    rig.halt(); pump.join();
    CHECK(rig.issued == range(0, 13) && rig.failures.empty());
    for (auto& report : rig.reports) CHECK(report.second);
    if (!early) CHECK(rig.reported_in_order(range(0, 13)));
    rig.check_rotation();
}

// copies land in reverse issue order, early reports off: nothing is reported until the oldest has landed, then all in issue order
static void reverse_without_early_reports() {
    Rig rig(4, 4);
    std::thread pump = rig.start(false);
    rig.push(0, 4);
    rig.await([&] { return rig.issued.size() == 4; });
    for (int job = 3; job >= 1; job--) rig.land(job);
    { std::lock_guard<std::mutex> lock(rig.mutex); CHECK(rig.reports.empty() && rig.in_lane[0] == 0); }   // (the pump asks nothing of the landed lanes: it waits for job 0)
    rig.land(0);
    rig.await([&] { return rig.reports.size() == 4; });
    rig.halt(); pump.join();
    CHECK(rig.reported_in_order(range(0, 4)));
    rig.check_rotation();
}

// the same with early reports, the thread held in the third job's readiness wait: the later lane's job is reported while the earlier
// one is still in flight
static void reverse_with_early_reports() {
    Rig rig(4, 3);
    rig.gate = 2;
    std::thread pump = rig.start(true);
    rig.push(0, 3);
    rig.await([&] { return rig.in_ready == 2; });
    rig.land(1);
    { std::lock_guard<std::mutex> lock(rig.mutex); CHECK(rig.reports.empty()); rig.gate_open = true; rig.moved.notify_all(); }
    rig.await([&] { return rig.reports.size() == 1; });
    { std::lock_guard<std::mutex> lock(rig.mutex); CHECK(rig.reports[0].first == 1 && rig.in_lane[0] == 0); }
    rig.land(0); rig.land(2);
    rig.await([&] { return rig.reports.size() == 3; });
    rig.halt(); pump.join();
    CHECK(rig.issued == range(0, 3));
    rig.check_rotation();
}

// job 5 of 9 on two lanes is not ready (`at_issue`: is refused by the lanes). The owner's answer decides:
//   go on — told once, nothing issued for it, the lane it would have had goes to job 6, everything else completes;
//   end   — the thread returns by itself and issues nothing more. What the shared-memory publisher does at that point is kept: the
//           previous copy of the lane whose turn it was (job 3) has been finished and reported, the other lane's (job 4) is left in
//           flight, unreported, for the owner's tear-down.
static void failure(bool at_issue, bool go_on) {
    Rig rig(2, 9);
    (at_issue ? rig.refuse : rig.unready) = 5;
    rig.go_on = go_on;
    std::thread pump = rig.start(false);
    rig.push(0, 9);
    if (go_on) {
        rig.land_in_order(8);
        rig.await([&] { return rig.reports.size() == 8; });
        rig.halt(); pump.join();
        CHECK(rig.issued == range(0, 9, 5) && rig.reported_in_order(range(0, 9, 5)));
    } else {
        rig.land_in_order(5);
        pump.join();
        CHECK(rig.issued == range(0, 5) && rig.reported_in_order(range(0, 4)));
        CHECK(rig.in_lane[0] == 4 && rig.in_lane[1] == -1 && rig.queue.size() == 3);
    }
    CHECK(rig.failures == std::vector<int>{5});
    rig.check_rotation();
}

// a copy that ends as a failure is reported as landed-but-failed, and the pump goes on
static void failed_copy() {
    Rig rig(2, 6);
    rig.bad[2] = 1;
    std::thread pump = rig.start(true);
    rig.push(0, 6);
    rig.land_in_order(6);
    rig.await([&] { return rig.reports.size() == 6; });
    rig.halt(); pump.join();
    for (auto& report : rig.reports) CHECK(report.second == (report.first != 2));
    CHECK(rig.failures.empty() && rig.issued == range(0, 6));
    rig.check_rotation();
}

// a job the owner's issue hook accounts for itself takes no lane and is no failure
static void skipped_job() {
    Rig rig(2, 6);
    rig.skip = 3;
    std::thread pump = rig.start(true);
    rig.push(0, 6);
    rig.land_in_order(5);
    rig.await([&] { return rig.reports.size() == 5; });
    rig.halt(); pump.join();
    CHECK(rig.issued == range(0, 6, 3) && rig.failures.empty());
    rig.check_rotation();                            // (job 4 on the lane job 3 would have had)
}

// stopped with four jobs queued and two copies in flight: all six are carried out and finished before the thread returns
static void stop_with_work() {
    Rig rig(2, 6);
    std::thread pump = rig.start(false);
    rig.push(0, 6);
    rig.await([&] { return rig.issued.size() == 2; });
    rig.halt();
    rig.land_in_order(6);
    pump.join();
    CHECK(rig.reported_in_order(range(0, 6)));
    for (int lane = 0; lane < 2; lane++) CHECK(rig.in_lane[lane] < 0);
    rig.check_rotation();
}

static void stop_while_asleep() {
    Rig rig(4, 0);
    std::thread pump = rig.start(true);
    rig.await([&] { return rig.sleeping; });
    rig.halt(); pump.join();
    CHECK(rig.issued.empty() && rig.reports.empty());
}

// 2 000 jobs from a producer that pauses at random, copies that land in random order among those in flight
static void storm(bool early) {
    const int jobs = 2000;
    Rig rig(4, jobs);
    std::thread pump = rig.start(early);
    std::thread producer([&] {
        std::mt19937 random(early ? 11 : 12);
        for (int job = 0; job < jobs; job++) {
            rig.push(job, 1);
            const unsigned pause = random() % 8;
            if (pause == 0) std::this_thread::sleep_for(std::chrono::microseconds(random() % 40));
            else if (pause < 3) std::this_thread::yield();
        }
    });
    std::thread lander([&] {
        std::mt19937 random(early ? 21 : 22);
        std::vector<int> flying;
        size_t seen = 0;
        for (int landed = 0; landed < jobs; landed++) {
            {
                std::unique_lock<std::mutex> lock(rig.mutex);
                rig.moved.wait(lock, [&] { return !flying.empty() || rig.issued.size() > seen; });
                while (seen < rig.issued.size()) flying.push_back(rig.issued[seen++]);
            }
            const size_t pick = random() % flying.size();
            rig.land(flying[pick]);
            flying.erase(flying.begin() + (long)pick);
            if (random() % 4 == 0) std::this_thread::yield();
        }
    });
    producer.join(); lander.join();
    rig.await([&] { return rig.reports.size() == (size_t)jobs; });
    rig.halt(); pump.join();
    CHECK(rig.issued == range(0, jobs) && rig.failures.empty());
    if (!early) CHECK(rig.reported_in_order(range(0, jobs)));
    rig.check_rotation();
}

int main() {
    for (int lanes : {1, 2, 4}) for (bool early : {false, true}) run("thirteen jobs", [&] { turns(lanes, early); });
    run("reverse landing, reports in issue order", reverse_without_early_reports);
    run("reverse landing, early reports", reverse_with_early_reports);
    for (bool at_issue : {false, true}) for (bool go_on : {true, false})
        run(at_issue ? (go_on ? "issue fails, go on" : "issue fails, end") : (go_on ? "not ready, go on" : "not ready, end"), [&] { failure(at_issue, go_on); });
    run("a copy fails", failed_copy);
    run("a job that takes no lane", skipped_job);
    run("stop with jobs queued and copies in flight", stop_with_work);
    run("stop while asleep", stop_while_asleep);
    for (bool early : {false, true}) run(early ? "storm, early reports" : "storm, reports in issue order", [&] { storm(early); });
    return 0;
}
