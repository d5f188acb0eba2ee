// RCCL through dlopen (rccl_dyn.h): the library and its entry points, resolved once, and the process-wide cache of communicators — shared by
// the row-range shards of float_vector indexes (rxgpu_sharded.hip) and the document-range shards of ft_fast (rxgpu_ft_sharded.hip).
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>

#include <hip/hip_runtime.h>
#include "rccl_dyn.h"   // <rccl/rccl.h> for types and prototypes only: the library is opened at the first sharded index (rccl_api below)

namespace rxgpu {

const RcclApi& rccl_api() {
	static RcclApi api;
	static std::once_flag once;
	std::call_once(once, [] {
		void* lib = nullptr;
		std::string tried;
		const char* env = std::getenv("RXGPU_RCCL_LIB");   // an explicit path (tests use it to provoke the fallback)
		const char* names[] = {env, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
		for (const char* n : names) {
			if (!n || !*n) continue;
			lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
			if (lib) break;
			const char* e = dlerror();
			tried += std::string(tried.empty() ? "" : "; ") + n + ": " + (e ? e : "?");
			if (n == env) break;   // an explicit choice is not second-guessed
		}
		if (!lib) {
			api.why = "librccl.so could not be opened (" + tried + ")";
			return;
		}
		auto sym = [&](const char* name) -> void* {
			void* p = dlsym(lib, name);
			if (!p && api.why.empty()) api.why = std::string("librccl.so lacks ") + name;
			return p;
		};
		api.ncclCommInitAll = reinterpret_cast<decltype(api.ncclCommInitAll)>(sym("ncclCommInitAll"));
		api.ncclAllGather = reinterpret_cast<decltype(api.ncclAllGather)>(sym("ncclAllGather"));
		api.ncclGroupStart = reinterpret_cast<decltype(api.ncclGroupStart)>(sym("ncclGroupStart"));
		api.ncclGroupEnd = reinterpret_cast<decltype(api.ncclGroupEnd)>(sym("ncclGroupEnd"));
		api.ncclGetErrorString = reinterpret_cast<decltype(api.ncclGetErrorString)>(sym("ncclGetErrorString"));
	});
	return api;
}

std::shared_ptr<RcclCommSet> rccl_comm_set(const std::vector<int>& devices, std::string* why) {
	static std::mutex pool_mtx;
	static std::vector<std::shared_ptr<RcclCommSet>>* pool = new std::vector<std::shared_ptr<RcclCommSet>>();   // never torn down: no RCCL calls at exit
	const RcclApi& api = rccl_api();
	if (!api.why.empty()) {
		if (why) *why = "RCCL unavailable: " + api.why;
		return nullptr;
	}
	std::lock_guard<std::mutex> lk(pool_mtx);
	for (const auto& cs : *pool) {
		if (cs->devices == devices) return cs;
	}
	auto cs = std::make_shared<RcclCommSet>();
	cs->devices = devices;
	cs->comms.assign(devices.size(), nullptr);
	int prev = -1;
	(void)hipGetDevice(&prev);
	const ncclResult_t nr = api.ncclCommInitAll(cs->comms.data(), int(devices.size()), devices.data());
	if (prev >= 0) (void)hipSetDevice(prev);
	if (nr != ncclSuccess) {
		if (why) *why = std::string("ncclCommInitAll over ") + std::to_string(devices.size()) + " device(s): " + api.ncclGetErrorString(nr);
		return nullptr;
	}
	pool->push_back(cs);
	return cs;
}

}  // namespace rxgpu
