/*
 * hls_stream.h -- stand-in for the Vitis HLS header (own text; see ap_fixed.h).  A stream is an unbounded FIFO.  The
 * reference's dataflow regions run here as plain sequential calls, producer before consumer, so a write never has to
 * wait; a read from an empty stream could only wait for ever, so it ends the program with a message instead.
 */
#ifndef HLS_STANDIN_HLS_STREAM_H
#define HLS_STANDIN_HLS_STREAM_H

#include <cstdio>
#include <cstdlib>
#include <deque>

namespace hls {
template <typename T>
class stream {
public:
    stream() : name_("stream") {}
    explicit stream(const char* name) : name_(name) {}
    stream(const stream&) = delete;
    stream& operator=(const stream&) = delete;
    bool empty() const { return q_.empty(); }
    bool full() const { return false; }
    unsigned size() const { return (unsigned)q_.size(); }
    void write(const T& x) { q_.push_back(x); }
    T read()
    {
        if (q_.empty()) {
            std::fprintf(stderr, "hls::stream stand-in: read from empty stream '%s'\n", name_);
            std::abort();
        }
        T x = q_.front();
        q_.pop_front();
        return x;
    }
    void read(T& x) { x = read(); }
    void operator<<(const T& x) { write(x); }
    void operator>>(T& x) { x = read(); }

private:
    const char* name_;
    std::deque<T> q_;
};
}  // namespace hls
#endif
