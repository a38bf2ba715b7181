// icp_host_check.cpp -- the owner of icp.hip's result mailbox and staging buffer (kfx::ResultPort) under the host sanitizers, on a
// machine without a device: construction, the refusals when nothing can be allocated, the sequence counter's wrap past 0 and the
// destruction of a thread's instance.  What enqueues or spins needs a device and is not covered here.
//   hipcc -std=c++17 -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined scripts/icp_host_check.cpp \
//       -o icp_host_check -pthread && HIP_VISIBLE_DEVICES=-1 ./icp_host_check
#include <cassert>
#include <cstdio>
#include <thread>

#include "../kangaroo_amd/csrc/icp.hip"

static int n_errors = 0, n_hooks = 0;
int kfx::set_error(int code, const char*) { ++n_errors; return code ? code : -1; }
int kfx::check_launch(const char*) { return 0; }
static void hook(void*) { ++n_hooks; }

int main()
{
    int devices = 0;
    if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) { puts("a device is visible: nothing checked"); return 0; }
    (void)hipGetLastError();
    {
        kfx::ResultPort port;
        assert(port.mailbox() == nullptr && port.mail == nullptr);   // no device: the copy path
        assert(port.mailbox() == nullptr);                             // ... at every call
        port.seq = 0xfffffffeu;
        assert(port.next_seq() == 0xffffffffu && port.next_seq() == 1u && port.next_seq() == 2u);   // never 0
        double r[15] = {}, src[15] = {};
        assert(port.read_back(r, src, sizeof(r), nullptr, nullptr, nullptr) != 0 && n_errors == 1);   // nothing to copy with
        assert(port.read_back(r, src, sizeof(r), nullptr, hook, nullptr) != 0 && n_errors == 2 && n_hooks == 0);   // no enqueue: no hook
        double T[12];
        float rmse = -1.f;
        unsigned obs = 7;
        int good = -1;
        const double res[15] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0.25, 42.0, 1.0};
        kfx::deliver(res, T, &rmse, &obs, &good);
        kfx::deliver(res, T, nullptr, nullptr, nullptr);
        assert(T[5] == 1.0 && rmse == 0.25f && obs == 42u && good == 1);
    }
    std::thread([] { assert(kfx::result_port.mailbox() == nullptr && kfx::result_port.next_seq() == 1u); }).join();   // its instance is destroyed at the thread's end
    assert(kfx::result_port.next_seq() == 1u);   // one per thread
    puts("icp_host_check: ok");
    return 0;
}
