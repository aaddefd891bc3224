// gicp_hostmath.h — the part of the host layer that makes no HIP call (gicp_hostmath.cpp): the tiling and its
// thread pool, the host scans, parameter defaults, the screen margins, the twist logarithm, the report's information
// matrix and eigensolver, the argument checks.
// Builds with the host compiler alone and links without the runtime (tests/native/host_check.cpp).
#pragma once

#include <cmath>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gicp_hip.h"
#include "gicp_internal.h"
#include "gicp_mem.h"

namespace gicp {

// A few persistent host threads for the tiling (spawning threads per cloud costs tens of us each,
// which a 100k-point frame of a stream cannot afford).  run(n, fn) calls fn(0 .. n-1) on the workers
// and the calling thread and returns when all are done; one caller at a time.
class WorkerPool {
public:
    explicit WorkerPool(int workers) {
        for (int i = 0; i < workers; ++i) th_.emplace_back([this] { loop(); });
    }
    ~WorkerPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void run(int tasks, std::function<void(int)> fn) {
        std::unique_lock<std::mutex> lk(m_);
        job_ = std::move(fn);
        ntasks_ = tasks;
        next_ = done_ = 0;
        ++gen_;
        lk.unlock();
        cv_.notify_all();
        work();
        lk.lock();
        done_cv_.wait(lk, [&] { return done_ == ntasks_ && active_ == 0; });
    }

private:
    void work() {
        for (;;) {
            int k;
            {
                std::lock_guard<std::mutex> g(m_);
                if (next_ >= ntasks_) return;
                k = next_++;
            }
            job_(k);
            std::lock_guard<std::mutex> g(m_);
            if (++done_ == ntasks_) done_cv_.notify_all();
        }
    }
    void loop() {
        std::unique_lock<std::mutex> lk(m_);
        long seen = 0;
        for (;;) {
            cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
            if (stop_) return;
            seen = gen_;
            ++active_;
            lk.unlock();
            work();
            lk.lock();
            if (--active_ == 0) done_cv_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::mutex m_;
    std::condition_variable cv_, done_cv_;
    std::function<void(int)> job_;
    int ntasks_ = 0, next_ = 0, done_ = 0, active_ = 0;
    long gen_ = 0;
    bool stop_ = false;
};

void default_params(int dim, gicp_params* p);
gicp_params resolve(int dim, const gicp_params* in);
Margin make_margin(int dim, float rho_q, float rho_db, double dmax);
float screen_bound(const Margin& m, double d);
double accept_d2_max(double dc);

void build_tile_table(const std::vector<uint32_t>& codes, int dim, int bits, std::vector<int32_t>& start,
                      std::vector<int32_t>& count, std::vector<uint32_t>& first_code, int& cap_out, int k_hint,
                      WorkerPool& pool, int maxp = kTile);
inline int tile_cap_of(int k) { return (int)(2.0 * std::pow(2.0, k / 4.0)); }   // extent cap of step k, in grid cells
int shard_tile_count(int ntiles, int shard, int nshards);
int build_seed_table(const std::vector<uint32_t>& tcode, int code_bits, std::vector<int32_t>& seed);

void scan_bounds(const double* xyz, int64_t n, int dim, double (&mn)[3], double (&mx)[3]);
void scan_stamps(const double* stamps, int64_t n, double ref);
double dec_ordered(unsigned long long e);
void decode_bounds(const unsigned long long* res, int dim, double (&mn)[3], double (&mx)[3]);

int voxel_key_bits(int dim, const double (&mn)[3], const double (&mx)[3], double leaf, double (&cmin)[3], int32_t (&bits)[3]);
int64_t map_window_cells(int dim, double leaf, double max_range, int& bits);
int64_t map_window_lo(int axis, double t, double leaf, int64_t R);

void motion_twist(int dim, const double* M, double* xi);
void deskew_host(const double* xyz, const double* stamps, int64_t n, int dim, const double* xi, double ref, double* out);

// input filters: the setting's checks, the grid of radius outlier removal, the host yardstick
void check_filter(const gicp_filter& f);
bool filter_crops(const gicp_filter& f);
[[noreturn]] void fail_filter_empty(int stage, int64_t n, const gicp_filter& f);
int ror_key_bits(int dim, const double (&mn)[3], const double (&mx)[3], double radius, double& leaf, double (&cmin)[3],
                 int32_t (&bits)[3], int64_t (&cmax)[3], const char* stage = "filter");
void check_filter_args(const double* xyz, int64_t N, int dim, const gicp_filter* f, const double* out_xyz, const int64_t* M_out);
void filter_points_host(const double* xyz, int64_t N, int dim, const gicp_filter* f, double* out_xyz, int64_t* out_index,
                        int32_t* out_count, int64_t* M_out);

// exact k-nearest-neighbour queries: the argument checks of every entry point, the host yardstick
void check_knn_args(const double* queries, int64_t Q, int dim, int k, double max_distance);
void knn_host(const double* xyz, int64_t M, const double* queries, int64_t Q, int dim, int k, double max_distance,
              int64_t* index, double* dist2, int32_t* count);

// statistical outlier removal: the setting's checks, what a stage refuses, the host yardstick
void check_sor(const gicp_sor& s);
void check_sor_args(const double* xyz, int64_t N, int dim, const gicp_sor* s, const int64_t* M_out, double (&mn)[3], double (&mx)[3]);
void check_sor_rows(int64_t m);
void check_sor_extent(int dim, const double (&mn)[3], const double (&mx)[3]);
void check_sor_result(double t_mean, int64_t kept, int64_t m, const gicp_sor& s);
void sor_points_host(const double* xyz, int64_t N, int dim, const gicp_sor* s, double* out_xyz, int64_t* out_index,
                     double* out_mean, double* out_stats, int64_t* M_out);

// Euclidean cluster extraction: the setting's checks, what a stage refuses, the host yardstick
void check_cluster(const gicp_cluster& c);
void check_cluster_args(const double* xyz, int64_t N, int dim, const gicp_cluster* c, double (&mn)[3], double (&mx)[3]);
void check_cluster_result(int64_t kept, int64_t m, int64_t clusters, const gicp_cluster& c);
void cluster_points_host(const double* xyz, int64_t N, int dim, const gicp_cluster* c, int32_t* labels, int32_t* sizes,
                         int64_t* n_clusters, double* out_xyz, int64_t* out_index, int64_t* M_out);

// registration report: information matrix of a pass's statistics, symmetric eigensolver
void information(int dim, const double* stats, const double* T, double* H, double* b);
void sym_eig(int n, const double* A, double* w, double* V);
void report_spectra(gicp_report* r);
int64_t quantile_rank(double pi, int64_t n);
void check_report_spec(const gicp_report_spec* spec, double dc);

void check_cloud_args(const double* xyz, int64_t n, int dim);
void check_shard(int shard, int nshards);
int current_failure(std::string& msg);
void set_host_error(const std::string& msg) noexcept;

}  // namespace gicp
