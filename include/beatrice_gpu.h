/*
 * beatrice_gpu.h — C-ABI of the MI355X parse+filter stage.
 *
 * This is the drop-in boundary between Beatrice's C++ host (capture backends,
 * PluginManager, PacketFilter callers) and the hand-written gfx950 kernels in
 * beatrice_amd/csrc/. Plain C types only: pointers, sizes, POD structs. No
 * exception crosses it; every entry point returns an int status
 * (0 = OK, otherwise a beatrice::ErrorCode value, include/beatrice/Error.hpp:11-26
 * of the reference) and bt_last_error() gives the message.
 *
 * What each entry point replaces in the reference (/root/reference, read-only):
 *
 *   bt_filter_compile   PacketFilter::addFilter + the per-packet priority sort and
 *                       per-packet expression re-parsing of applyFilters
 *                       (src/PacketFilter.cpp:19-31, :57-73, :330-372). Expressions
 *                       are parsed ONCE here with the reference's own stoi/getline
 *                       semantics; the device gets a POD program.
 *   bt_parse_filter     PacketFilter::applyFilters(const std::vector<Packet>&)
 *                       (src/PacketFilter.cpp:121-130) fused with the per-layer
 *                       ProtocolParser::parsePacket(slice, name) calls
 *                       (src/parser/ProtocolParser.cpp:69-95, :238-284) over a
 *                       host batch (pinned staging, H2D -> kernels -> D2H).
 *   bt_parse_filter_device  the same over device-resident buffers, async on a
 *                       caller stream (the hot path that bench.py measures).
 *   bt_extract_device / bt_extract
 *                       ProtocolParser::parsePacket(packet, ProtocolDefinition) and the
 *                       by-name form for registered user protocols
 *                       (src/parser/ProtocolParser.cpp:69-110, :238-433) over a batch;
 *                       bt_time_extract_ex times it (bench.py's c1 entry).
 *
 * Record layout (bt_rec, 96 B per packet). Each layer L found by the layer walk
 * (DESIGN.md "R-WALK") has the field values that
 *   ProtocolParser(enablePerformanceMetrics=false).parsePacket(
 *       std::vector<uint8_t>(frame + off_L, frame + len), L)
 * returns, bit for bit: integers are the reference's extractValue<T> results
 * (big-endian wire order decoded, src/parser/ProtocolParser.cpp:418-431) stored
 * little-endian; BYTES / IPV4_ADDRESS / IPV6_ADDRESS fields are the raw bytes.
 * A layer whose slice is shorter than its table's getTotalLength() has status
 * PACKET_TOO_SHORT and no fields (:244-247): its field bytes are zero here.
 * Bytes of absent layers and reserved bytes are zero. Bytes 88..90 hold the
 * ProtocolDetector column of the whole frame (BT_DET_* / BT_IS_* below).
 *
 * On the device the records are PACKED and stored tiled by 64 packets (one wavefront
 * tile), SoA by 16-byte slab inside the tile: slab k (k = 0..5) of packet i lives at
 *     records + ((i / 64) * 6 + k) * 1024 + (i % 64) * 16
 * so each wavefront store instruction writes 1 KiB contiguously. The buffer needs
 * ceil(n / 64) * 6144 bytes. BT_OPT_RECORDS_PLANES selects plane-major slabs instead:
 * (k * n_cap + i) * 16. A packed record holds only the fields of the layers that
 * parsed (bt_rec.ok), each right after the previous one, as 24 little-endian dwords c[]:
 *   c0..c3  = bt_rec bytes 0..15 (Ethernet, pkt_len)
 *   c4      = present | ok << 8 | detect_code << 16 (3 bits) | detect_is << 19 (8 bits)
 *             | detect_is2 << 27 (3 bits); l3_off / l4_off are implied by present (+ IHL)
 *   then, per VLAN tag that parsed: vlan_tci[0] | vlan_tpid[1] << 16, then vlan_tci[1]
 *             (vlan_tpid[0] is the ethertype)
 *   then L3: IPv4 b0 | tos << 8 | ttl << 16 | protocol << 24, total_length | id << 16,
 *            flags | checksum << 16, source_ip, destination_ip (version == ihl == b0);
 *            or IPv6 as bt_rec bytes 28..67
 *   then L4: TCP 5 dwords / UDP, ICMP 2 dwords, as bt_rec bytes 68..
 * A record needs ceil(dwords / 4) slabs (bt_record_slabs): untagged Eth/IPv4/UDP 3,
 * IPv4/TCP or one tag 4, IPv6/TCP + QinQ 6, no IP 2. In the tiled layout, slabs 0 and 1
 * of packet i are at the addresses above; slab k >= 2 is stored only by the packets that
 * need it, packed in packet order to the front of the tile's slab-k region (a packet's
 * slot = its rank among them; the last tile's unused slots hold a zero slab 1). In the
 * plane-major layout slab k is at the packet's slot, written for the whole wavefront
 * when any packet needs it. Bytes no packet needs are left as they were.
 * bt_record_gather() / bt_record_unpack() rebuild the bt_rec, which is the parity unit.
 */
#ifndef BEATRICE_GPU_H
#define BEATRICE_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history: 1 = round 1-3. 2 = round 4: a descriptor batch must state bt_batch.bytes
 * (0 was "unbounded" before and is now BT_E_INVALID_ARGUMENT); bt_group_host_register /
 * bt_group_parse_filter_mapped / bt_group_split_cost / bt_context_placement added. Hosts
 * built against an older header should check bt_abi_version() >= the version they need.
 * Added within 2 (new entry points only, nothing existing changed; a host that needs them can
 * look the symbols up): bt_filter_resume_device, bt_ring_stage_tpv3_ex, bt_pass_pack_device,
 * bt_pcap_index, bt_pcap_filter, bt_tally_device, bt_flow_fanout_device, bt_flow_hash_host,
 * bt_flow_table_scratch_bytes, bt_flow_table_device, bt_flow_table_host, bt_flow_track_layout,
 * bt_flow_track_scratch_bytes, bt_flow_track_expire_scratch_bytes, bt_flow_track_init_device,
 * bt_flow_track_update_device, bt_flow_track_expire_device, bt_flow_track_init_host,
 * bt_flow_track_update_host, bt_flow_track_expire_host, bt_flow_track_forget,
 * bt_flow_tcp_update_device, bt_flow_tcp_update_host, bt_flow_tcp_state,
 * bt_flow_track_expire_tcp_scratch_bytes, bt_flow_track_expire_tcp_device,
 * bt_flow_track_expire_tcp_host, bt_flow_track_top_scratch_bytes, bt_flow_track_top_device,
 * bt_flow_track_top_host, bt_flow_track_hosts_scratch_bytes, bt_flow_track_hosts_device,
 * bt_flow_track_hosts_host, bt_flow_stat_update_device, bt_flow_stat_update_host,
 * bt_flow_stat_rtt, bt_flow_track_side_move_scratch_bytes, bt_flow_track_side_move_device,
 * bt_flow_track_side_move_host, bt_flow_mark_update_device, bt_flow_mark_update_host,
 * bt_flow_mark_select_device, bt_flow_mark_select_host, bt_flow_seq_scratch_bytes,
 * bt_flow_seq_device, bt_flow_seq_host, bt_flow_stream_compile, bt_flow_stream_scratch_bytes,
 * bt_flow_stream_device, bt_flow_stream_host, bt_flow_tcpseq_scratch_bytes, bt_flow_tcpseq_device,
 * bt_flow_tcpseq_host, bt_flow_reasm_scratch_bytes, bt_flow_reasm_device, bt_flow_reasm_host,
 * bt_flow_follow_scratch_bytes, bt_flow_follow_device, bt_flow_follow_host. */
#define BT_ABI_VERSION 2

/* ---- status codes (values of beatrice::ErrorCode, reference include/beatrice/Error.hpp:11-26) */
#define BT_OK                    0
#define BT_E_INVALID_ARGUMENT    1
#define BT_E_INIT_FAILED         2
#define BT_E_RESOURCE            3
#define BT_E_INTERNAL           10
#define BT_E_NOT_IMPLEMENTED    11

/* ---- packet descriptor: byte offset (48 bits) | length (16 bits) << 48 -------- */
typedef uint64_t bt_pkt_desc;
#define BT_DESC(off, len) ((uint64_t)(off) | ((uint64_t)(len) << 48))
#define BT_DESC_OFF(d)    ((uint64_t)(d) & 0xFFFFFFFFFFFFull)
#define BT_DESC_LEN(d)    ((uint32_t)((uint64_t)(d) >> 48))

/* ---- parsed record --------------------------------------------------------- */
#define BT_REC_BYTES  96
#define BT_REC_SLABS  6

/* bt_rec.present / bt_rec.ok bits: layer attempted by the walk / status SUCCESS */
#define BT_L_ETH   0x01u
#define BT_L_VLAN0 0x02u
#define BT_L_VLAN1 0x04u
#define BT_L_IPV4  0x08u
#define BT_L_IPV6  0x10u
#define BT_L_TCP   0x20u
#define BT_L_UDP   0x40u
#define BT_L_ICMP  0x80u

/* bt_rec.detect_*: reference ProtocolDetector (src/parser/ProtocolRegistry.cpp:353-484)
 * applied to the whole frame. detect_code is detectProtocol(frame).protocolName:
 *   BT_DET_UNKNOWN   "unknown",  confidence 0.0,  reason "Packet too short"   (len < 14)
 *   BT_DET_NONE      "" / "" (the reference leaves confidence uninitialised)  (:356-357)
 *   BT_DET_ETHERNET  "ethernet", 0.95, "Valid Ethernet frame"
 *   BT_DET_TCP/UDP/ICMP  "tcp"/"udp"/"icmp", 0.98, "Ethernet + IPv4 + TCP|UDP|ICMP"
 *                    (frame byte 23 once len >= 34, whatever the EtherType)
 * detect_is: isEthernet, isIPv4, isIPv6, isTCP, isUDP, isICMP, isHTTP, isDNS (:418-480;
 * the IPv4/IPv6 tests read the version nibble of frame byte 0, as the reference does).
 * detect_is2: isARP (:482-487) and the second entry of detectMultipleProtocols (:390-416). */
#define BT_DET_UNKNOWN  0u
#define BT_DET_NONE     1u
#define BT_DET_ETHERNET 2u
#define BT_DET_TCP      3u
#define BT_DET_UDP      4u
#define BT_DET_ICMP     5u
#define BT_IS_ETHERNET  0x01u
#define BT_IS_IPV4      0x02u
#define BT_IS_IPV6      0x04u
#define BT_IS_TCP       0x08u
#define BT_IS_UDP       0x10u
#define BT_IS_ICMP      0x20u
#define BT_IS_HTTP      0x40u
#define BT_IS_DNS       0x80u
#define BT_IS2_ARP       0x01u
#define BT_IS2_MULTI_TCP 0x02u   /* detectMultipleProtocols adds {"tcp", 0.98, "TCP over IPv4"} */
#define BT_IS2_MULTI_UDP 0x04u   /* ... {"udp", 0.98, "UDP over IPv4"}                          */

#pragma pack(push, 1)
typedef struct bt_ipv4_fields {   /* reference src/parser/ProtocolRegistry.cpp:161-178 */
    uint8_t  version;             /* raw byte 0 (quirk: same byte as ihl)              */
    uint8_t  ihl;                 /* raw byte 0                                         */
    uint8_t  tos;
    uint8_t  ttl;
    uint8_t  protocol;
    uint8_t  _pad0;
    uint16_t total_length;
    uint16_t identification;
    uint16_t flags;               /* raw 16-bit flags + fragment offset                 */
    uint16_t checksum;
    uint16_t _pad1;
    uint8_t  source_ip[4];
    uint8_t  destination_ip[4];
    uint8_t  _pad2[16];
} bt_ipv4_fields;                 /* 40 B */

typedef struct bt_ipv6_fields {   /* reference src/parser/ProtocolRegistry.cpp:180-192 */
    uint32_t version_traffic_class_flow_label;
    uint16_t payload_length;
    uint8_t  next_header;
    uint8_t  hop_limit;
    uint8_t  source_ip[16];
    uint8_t  destination_ip[16];
} bt_ipv6_fields;                 /* 40 B */

typedef struct bt_tcp_fields {    /* reference src/parser/ProtocolRegistry.cpp:194-209 */
    uint16_t source_port;
    uint16_t destination_port;
    uint32_t sequence_number;
    uint32_t acknowledgment_number;
    uint8_t  data_offset;         /* raw byte 12 */
    uint8_t  flags;               /* raw byte 13 */
    uint16_t window_size;
    uint16_t checksum;
    uint16_t urgent_pointer;
} bt_tcp_fields;                  /* 20 B */

typedef struct bt_udp_fields {    /* reference src/parser/ProtocolRegistry.cpp:211-221 */
    uint16_t source_port;
    uint16_t destination_port;
    uint16_t length;
    uint16_t checksum;
    uint8_t  _pad[12];
} bt_udp_fields;                  /* 20 B */

typedef struct bt_icmp_fields {   /* reference src/parser/ProtocolRegistry.cpp:223-234 */
    uint8_t  type;
    uint8_t  code;
    uint16_t checksum;
    uint16_t identifier;
    uint16_t sequence_number;
    uint8_t  _pad[12];
} bt_icmp_fields;                 /* 20 B */

typedef struct bt_rec {
    /* slab 0 */
    uint8_t  eth_destination_mac[6];   /* reference ProtocolRegistry.cpp:154 (BYTES) */
    uint8_t  eth_source_mac[6];        /* :155 (BYTES)                               */
    uint16_t eth_ethertype;            /* :156                                       */
    uint16_t pkt_len;                  /* min(frame length, 65535)                   */
    /* slab 1 */
    uint16_t vlan_tpid[2];             /* ProtocolRegistry.cpp:293 per tag           */
    uint16_t vlan_tci[2];              /* :294                                       */
    uint8_t  present;                  /* BT_L_* layers the walk attempted           */
    uint8_t  ok;                       /* BT_L_* layers with ParseStatus::SUCCESS    */
    uint8_t  l3_off;                   /* frame offset of the L3 slice (0 if none)   */
    uint8_t  l4_off;                   /* frame offset of the L4 slice (0 if none)   */
    /* slabs 1..4: L3 union at 28, L4 union at 68 */
    union { bt_ipv4_fields ipv4; bt_ipv6_fields ipv6; } l3;
    union { bt_tcp_fields tcp; bt_udp_fields udp; bt_icmp_fields icmp; } l4;
    /* slab 5 tail: the ProtocolDetector column for the whole frame */
    uint8_t  detect_code;              /* BT_DET_*: detectProtocol(frame)            */
    uint8_t  detect_is;                /* BT_IS_* predicate bits                     */
    uint8_t  detect_is2;               /* BT_IS2_* bits                              */
    uint8_t  _reserved[5];
} bt_rec;
#pragma pack(pop)

/* ---- filters --------------------------------------------------------------- */
/* Same enumerator order as beatrice::PacketFilter::FilterType
 * (reference include/beatrice/PacketFilter.hpp:17-24). */
enum bt_filter_type {
    BT_FILTER_BPF = 0,
    BT_FILTER_PROTOCOL = 1,
    BT_FILTER_IP_RANGE = 2,
    BT_FILTER_PORT_RANGE = 3,
    BT_FILTER_PAYLOAD = 4,
    BT_FILTER_CUSTOM = 5
};

typedef struct bt_filter_desc {       /* mirrors PacketFilter::FilterConfig hpp:26-33 */
    int32_t     type;                  /* enum bt_filter_type                          */
    const char* expression;            /* NUL-terminated; NULL == ""                   */
    int32_t     enabled;
    int32_t     priority;              /* higher = evaluated first                      */
    int32_t     has_custom_func;       /* CUSTOM only: a std::function is installed     */
} bt_filter_desc;

/* compiled filter kinds (device program) */
enum bt_filter_kind {
    BT_K_TRUE = 0,        /* empty expression (every apply*Filter :169,194,220,250,289) or unset CUSTOM */
    BT_K_FALSE = 1,       /* can only ever return false                                           */
    BT_K_BPF = 2,         /* substring keywords tcp/udp/icmp (:168-191)                           */
    BT_K_PROTO_EQ = 3,    /* "tcp"/"udp"/"icmp" (:210-212)                                        */
    BT_K_PROTO_NZ = 4,    /* "ip" (:213)                                                          */
    BT_K_IP_MASK = 5,     /* CIDR or exact dotted quad (:219-247, :342-360)                       */
    BT_K_PORT = 6,        /* inclusive range or exact port (:249-286, :362-372)                   */
    BT_K_IP_THROW = 7,    /* expression makes std::stoi throw once the IPv4 gates pass            */
    BT_K_PORT_THROW = 8,  /* same for the port filter once the TCP/UDP length gates pass          */
    BT_K_HOST = 9,        /* PAYLOAD regex outside the DFA subset / installed CUSTOM callback:    */
                          /* evaluated on the host                                                */
    BT_K_PAYLOAD = 10     /* PAYLOAD regex compiled to a byte DFA (bt_payload_dfa_compile):       */
                          /* a = byte offset of its blob in the context's DFA pool, b = blob size */
};

typedef struct bt_filter_slot {       /* one compiled program slot, in evaluation order */
    uint32_t source_index;            /* index into the bt_filter_desc array            */
    uint32_t kind;                    /* enum bt_filter_kind                            */
    uint32_t a, b;                    /* kind parameters                */
    int32_t  throw_kind;              /* 0 none, 1 std::invalid_argument, 2 std::out_of_range */
} bt_filter_slot;

#define BT_MAX_FILTERS 64

/* Per-packet decision byte: (code << 6) | slot. */
#define BT_DECIDE_PASS   0u   /* every enabled filter returned true (slot = last slot, 0 if none) */
#define BT_DECIDE_REJECT 1u   /* slot = first filter that returned false                           */
#define BT_DECIDE_THROW  2u   /* slot = filter whose expression throws (reference rethrows)        */
#define BT_DECIDE_HOST   3u   /* slot = first host-only filter reached; host continues from there  */
#define BT_DECIDE_CODE(x) ((uint32_t)(x) >> 6)
#define BT_DECIDE_SLOT(x) ((uint32_t)(x) & 63u)

/* ---- context --------------------------------------------------------------- */
typedef struct bt_ctx bt_ctx;

typedef struct bt_opts {
    uint32_t host_chunk_packets;   /* bt_parse_filter pipeline chunk (0 = default 1M)  */
    uint32_t host_chunk_bytes;     /* pinned staging bytes per chunk (0 = default 256 MiB) */
    uint32_t grid_waves;           /* 0 = auto (persistent grid sized to the device)    */
    uint32_t flags;                /* BT_OPT_*                                          */
    uint32_t host_threads;         /* host-path threads (0 = auto: BT_HOST_THREADS, else the
                                      usable CPUs (affinity, cgroup quota)); <= 16; a host
                                      batch uses <= 8 of them while others wait for the context */
    uint32_t reserved[3];
} bt_opts;

#define BT_OPT_NO_PREFETCH 0x1u    /* disable the next-tile load prefetch (A/B only)    */
#define BT_OPT_TILE_BLOCKED 0x2u   /* one contiguous tile range per wavefront           */
#define BT_OPT_RECORDS_AOS 0x4u    /* device records as bt_rec AoS instead of planes    */
#define BT_OPT_GRAPH 0x8u          /* bt_time_device: replay the steps as one hipGraph  */
#define BT_OPT_RECORDS_PLANES 0x10u /* device records plane-major (k * n_cap + i) * 16  */
#define BT_OPT_NT_STORES 0x20u     /* force non-temporal record stores                   */
#define BT_OPT_NT_LOADS 0x40u      /* force non-temporal header loads                    */
#define BT_OPT_CACHE_DEFAULT 0x80u /* default cache policy everywhere (A/B only)         */
#define BT_OPT_SPIN_SYNC 0x100u    /* spin-wait host synchronisation (bench / latency)   */
#define BT_OPT_PAYLOAD_HOST 0x200u /* keep every PAYLOAD filter on the host (std::regex) */
#define BT_OPT_WIDE_NEVER 0x400u   /* descriptor mode: always two-round loads (A/B only)   */
#define BT_OPT_WIDE_ALWAYS 0x800u  /* descriptor mode: always wide round A (A/B only)      */
#define BT_OPT_PIPELINE 0x2000u    /* bt_time_device: steps as bt_parse_filter_device_async */
#define BT_OPT_GROUP_SHARED_DEVICE 0x4000u /* bt_group_create: allow a device listed more than once:
                                      that many lanes (contexts) on it; concurrent host batches
                                      then run whole on the least busy member (groups route a
                                      call that finds another in flight, up to
                                      BT_GROUP_ROUTE_BELOW packets, default 1M, instead of
                                      splitting it) */
#define BT_OPT_NO_LEAN_PCIE 0x8000u /* frames in host memory: read whole 64-B windows (A/B only) */
#define BT_OPT_MAPPED_GATHER_SPARSE 0x10000u /* bt_group_parse_filter_mapped, filter-only calls over
                                      bt_pkt_desc: a member whose frames lie far apart (sampled
                                      mean spacing >= BT_MAPPED_GATHER_ABOVE, default 512 B)
                                      gathers their prefixes on its host threads instead of
                                      reading each frame's window over PCIe */
#define BT_OPT_NO_LEAN_HOST 0x20000u /* host batches, filter-only: stage each frame's first 48 B
                                      instead of bytes 12..43 (A/B only) */
#define BT_OPT_PAYLOAD_DFA 0x40000u /* PAYLOAD slots as byte DFAs even where the bit-parallel
                                      form fits (A/B only) */
#define BT_OPT_PAYLOAD_EXTENDED 0x80000u /* PAYLOAD slots: also compile \b \B, POSIX bracket
                                      classes ([[:alpha:]]) and DFAs of up to 4,096 states for
                                      the GPU (BT_DFA_EXTENDED) instead of leaving them on the
                                      host; contexts and groups (opt-in: the default
                                      classification is unchanged) */

/* descriptor formats (bt_batch.desc_format) */
#define BT_DESC_PACKED 0u          /* bt_pkt_desc: u64 offset:48 | length:16            */
#define BT_DESC_XDP    1u          /* struct xdp_desc {u64 addr; u32 len; u32 options} as
                                      an AF_XDP RX ring holds it (linux/if_xdp.h), aligned
                                      chunk mode: addr = byte offset into the UMEM        */

typedef struct bt_batch {          /* input; device memory or host memory mapped with
                                      bt_host_register (zero-copy over PCIe)             */
    const uint8_t* base;           /* packet bytes (e.g. the UMEM)                      */
    const void* desc;              /* one descriptor per packet; NULL = fixed stride    */
    uint32_t stride;               /* fixed-stride mode: packet i = base[i*stride .. +stride) */
    uint32_t n;                    /* packets                                           */
    uint64_t bytes;                /* size of the base buffer (bounds check)            */
    uint32_t desc_format;          /* BT_DESC_PACKED / BT_DESC_XDP                      */
    uint32_t flags;                /* BT_BATCH_*                                        */
} bt_batch;

/* bt_batch.flags */
#define BT_BATCH_PREFIXES 0x1u     /* base holds header prefixes (bt_ring_gather_tpv3), not
                                      whole frames: PAYLOAD slots, which read past the
                                      headers, are left to the host (BT_DECIDE_HOST)     */
#define BT_BATCH_LEAN 0x2u         /* with BT_BATCH_PREFIXES: frame bytes 12..43 only
                                      (bt_ring_gather_lean_tpv3); records refused        */

typedef struct bt_outputs {        /* any pointer may be NULL = not produced            */
    void*     records;             /* ceil(n/64) * 6144 bytes, tiled slabs (see above)  */
    uint32_t  n_cap;               /* records capacity (>= n); plane stride with PLANES */
    uint64_t* verdict;             /* ceil(n/64) words, bit i%64 of word i/64 = passed  */
    uint8_t*  decide;              /* n bytes, BT_DECIDE_*                              */
    uint32_t* pass_idx;            /* n entries: indices of passing packets, ascending  */
    uint32_t* n_pass;              /* 1 word                                            */
} bt_outputs;

int  bt_abi_version(void);
const char* bt_last_error(void);              /* thread-local message of the last failure */

int  bt_create(int device, const bt_opts* opts, bt_ctx** out);
void bt_destroy(bt_ctx* ctx);
int  bt_device_count(int* out);
/* The context's device: its HIP ordinal and PCI bus id ("0000:05:00.0"; cap >= 16), so
 * that processes sharing a node can check they drive distinct GPUs. */
int  bt_context_device(const bt_ctx* ctx, int* device, char* pci_bus_id, uint32_t cap);
/* Where the context's host work runs: the host NUMA node closest to its device (HIP's
 * hipDeviceAttributeHostNumaId, else the PCI function's sysfs numa_node; -1 unknown), how
 * many CPUs of that node (in this process's affinity set) its pool workers are pinned to
 * (0 = not pinned; BT_NUMA_PIN=0 turns pinning off), the pool's size, and the node of the
 * host pipeline's pinned staging (-1 until a host batch allocated it). */
typedef struct bt_placement {
    int32_t  numa_node;
    uint32_t pinned_cpus;
    uint32_t pool_threads;
    int32_t  staging_node;
    uint32_t reserved[4];
} bt_placement;
int  bt_context_placement(bt_ctx* ctx, bt_placement* out);
/* Host-only: the CPUs this process may use (affinity set bounded by the cgroup v2 quota). */
uint32_t bt_usable_cpus(void);

/* Compile the enabled filters: stable sort by priority (descending), parse each
 * expression once. The C++ adapter (beatrice_amd/host) passes filters already in
 * the reference's own evaluation order so ties match libstdc++ exactly. */
int  bt_filter_compile(bt_ctx* ctx, const bt_filter_desc* filters, uint32_t n);
int  bt_filter_program(const bt_ctx* ctx, bt_filter_slot* out, uint32_t cap, uint32_t* n_slots);
/* The compiled program's PAYLOAD DFA tables (BT_K_PAYLOAD slot s: bytes [s.a, s.a + s.b) of
 * the pool, a blob for bt_payload_dfa_eval): *bytes = the pool's size, min(cap, size) bytes
 * copied to out. For hosts that evaluate small batches on the CPU with the same program. */
int  bt_filter_dfa_pool(const bt_ctx* ctx, void* out, uint32_t cap, uint32_t* bytes);

/* Pre-size the device workspace for batches of up to n packets (so later launches
 * never allocate, e.g. under hipGraph capture). */
int  bt_reserve(bt_ctx* ctx, uint32_t n);

/* Device-resident parse+filter, asynchronous on `stream` (a hipStream_t, NULL =
 * the context's own stream). records != NULL selects parsing; the filter
 * outputs are produced when any of verdict/decide/pass_idx/n_pass is set. */
int  bt_parse_filter_device(bt_ctx* ctx, const bt_batch* batch, const bt_outputs* out, void* stream);

/* Second pass for a batch first run with BT_BATCH_PREFIXES: `frames` holds the WHOLE frames of
 * the same n packets, in the same order (flags must not have BT_BATCH_PREFIXES); out->decide
 * holds the first pass's n decision bytes and is rewritten in place. out->verdict (optional):
 * all ceil(n/64) words rebuilt from the final decision bytes; out->pass_idx / n_pass
 * (optional): the ordered pass list from them. out->records must be NULL. Asynchronous on
 * `stream` (NULL = the context's stream), after which the outputs equal those of
 * bt_parse_filter_device over `frames`. A program without a BT_K_PAYLOAD slot: only the
 * optional verdict / pass list are rebuilt.
 * The pass takes every decision left as BT_DECIDE_HOST at a BT_K_PAYLOAD slot s (the first pass
 * could not read the payload), evaluates slots s .. n-1 over the whole frame on the GPU and
 * rewrites the byte; every other byte, BT_DECIDE_HOST at a BT_K_HOST slot included, is left as
 * it is. It reads frame bytes 12..37 and the PAYLOAD window, each 16-B chunk under the rule of
 * bt_parse_filter_device (a chunk past `bytes` reads as zeros). BT_E_INVALID_ARGUMENT: a null
 * argument, BT_BATCH_PREFIXES / BT_BATCH_LEAN set, records != NULL, decide == NULL, a
 * descriptor batch with bytes == 0. */
int  bt_filter_resume_device(bt_ctx* ctx, const bt_batch* frames, const bt_outputs* out, void* stream);

/* ---- the packets that passed: ordered pack of the selected frames ------------------
 * Every path above ends in a verdict; this one produces the frames. The selected packets'
 * bytes are packed in packet order into one buffer, on the GPU, so that only the survivors
 * cross PCIe (or go on to the next stage). `select` has the verdict-word layout (bit i % 64
 * of word i / 64; out->verdict of a filter call is one), device-visible like the rest; bits
 * at or above n in the last word are ignored.
 *   record k  = the k-th set bit's packet: `lead` bytes in front of the frame, then
 *               min(len, snap ? snap : len) frame bytes;
 *   its slot  = that size rounded up to `align`; the bytes between a record's end and its
 *               slot's end are written as zeros;
 *   its place = the sum of the earlier slots (64-bit).
 * Source bytes outside [0, frames->bytes) read as zeros (a lead in front of the buffer, a
 * descriptor running past it): the rule of bt_parse_filter_device; the kernel never reads
 * outside the buffer. A slot is written only when it ends at or below `cap`: nothing is ever
 * written at or past cap, *n_packed = the records of the longest prefix of the selection
 * whose slots all fit (whole records only), and *total = the bytes the whole selection needs,
 * whether it fits or not (total <= cap: everything was packed). Descriptor batches in both
 * formats and fixed-stride batches (frame length min(stride, 65535)) are taken.
 * BT_E_INVALID_ARGUMENT: a null argument (out->desc may be NULL; out->bytes may be NULL when
 * cap is 0, a size query), lead > 64, align not 1, 16 or 64, BT_BATCH_PREFIXES / BT_BATCH_LEAN
 * set (those batches hold no whole frames), a descriptor batch with bytes == 0.
 * Asynchronous on `stream` (NULL = the context's stream); two kernel launches, no allocation
 * once bt_reserve(n) has been called. */
typedef struct bt_pack_opts {
    uint32_t lead;     /* bytes in front of each frame copied with it (0..64): 16 over a pcap
                          file takes each record header along                               */
    uint32_t snap;     /* 0 = whole frames, else at most snap bytes of each frame            */
    uint32_t align;    /* 1, 16 or 64: every output record (lead + frame) starts on a multiple;
                          gap bytes are written as zeros                                     */
    uint32_t reserved;
} bt_pack_opts;
typedef struct bt_pack_out {           /* device-visible memory                              */
    uint8_t*     bytes;  uint64_t cap; /* packed output and its capacity                      */
    bt_pkt_desc* desc;                 /* optional, n entries: entry k = BT_DESC(offset of record
                                          k's frame (after its lead) in `bytes`, copied length),
                                          for every selected packet, in order: with n_packed a
                                          descriptor batch over `bytes`                       */
    uint64_t*    total;                /* bytes the whole selection needs (even when > cap)   */
    uint32_t*    n_packed;             /* records written: the longest prefix of the selection
                                          that fits in cap, whole records only                */
} bt_pack_out;
int  bt_pass_pack_device(bt_ctx* ctx, const bt_batch* frames, const uint64_t* select,
                         const bt_pack_opts* opts, const bt_pack_out* out, void* stream);

/* ---- counts of a batch that stays on the device -------------------------------------
 * What PacketFilter::getStats() (reference src/PacketFilter.cpp:374-386) and
 * ProtocolParser::getStats() (src/parser/ProtocolParser.cpp:174-182) answer, for a batch whose
 * per-packet outputs never cross PCIe: the decision bytes of a filter call counted by code and
 * by deciding slot, the frame lengths summed by code, and the parsed layers counted from the
 * records' present / ok bits. Only these 2,304 bytes go to the host.
 *   decide   the n decision bytes of a filter call (out->decide), device-visible, any
 *            alignment; NULL when only the layer counts are wanted.
 *   frames   optional: the batch the decisions belong to (frames->n == n). Only lengths are
 *            read, never frame bytes: both descriptor formats, and fixed stride with length
 *            min(stride, 65535) as in the pack. Without `decide` it is not read at all.
 *   records  optional: the records of the same call in the context's own layout (tiled, or
 *            BT_OPT_RECORDS_PLANES with plane stride n_cap, or BT_OPT_RECORDS_AOS); only the
 *            present | ok << 8 dword of packets [0, n) is read.
 * Without BT_TALLY_ACCUMULATE every byte of *out is written (sums whose input is NULL are 0).
 * With it n, scanned, code, slot, bytes and layer_* are added to what *out holds (a stream of
 * batches into one tally, read once per reporting interval); the four first_* fields always
 * describe this call alone. BT_DECIDE_HOST never stops the count. With BT_TALLY_STOP_AT_THROW,
 * scanned == first_throw and code[BT_DECIDE_THROW] == 0; the layer counts always cover [0, n).
 * All counts are exact. Asynchronous on `stream` (NULL = the context's stream), no host
 * synchronisation, two kernel launches (none for n == 0, which still writes *out on the
 * stream), no allocation once bt_reserve(n) has been called; usable right behind
 * bt_parse_filter_device on the same stream. The kernels read nothing outside the 16-byte
 * granules that hold decide[0 .. n), no descriptor at or past n and no record tile at or past
 * ceil(n / 64). BT_E_INVALID_ARGUMENT: a null context or out (or an out that is not 8-byte
 * aligned), decide and records both NULL, frames->n != n or a batch bt_parse_filter_device
 * refuses, records with n_cap < n, unknown flag bits. */
#define BT_TALLY_STOP_AT_THROW 0x1u  /* count only the packets before the first BT_DECIDE_THROW,
                                        as applyFilters(vector) / classify leave the stats      */
#define BT_TALLY_ACCUMULATE    0x2u  /* add to the counts already in *out (a stream of batches)  */

typedef struct bt_tally {            /* 2,304 B, device-visible memory, 8-byte aligned           */
    uint64_t n;                      /* packets of the batch(es)                                 */
    uint64_t scanned;                /* packets counted below: n, or the first throw's index     */
    uint64_t first_throw;            /* index of the first THROW decision in [0, n); n = none    */
    uint64_t first_host;             /* index of the first HOST decision in [0, n); n = none     */
    uint32_t first_throw_slot, first_host_slot;   /* their slots (0 when none)                   */
    uint64_t code[4];                /* decisions of [0, scanned) by BT_DECIDE_* code            */
    uint64_t slot[4][64];            /* ... by code and deciding slot                            */
    uint64_t bytes[4];               /* frame lengths of [0, scanned) summed by code             */
    uint64_t layer_present[8];       /* over [0, n): packets with bit k of bt_rec.present        */
    uint64_t layer_ok[8];            /* ... with bit k of bt_rec.ok                              */
    uint64_t reserved[3];            /* written as 0                                             */
} bt_tally;

int  bt_tally_device(bt_ctx* ctx, const uint8_t* decide, uint32_t n,
                     const bt_batch* frames,     /* optional: only lengths are read -> bytes[]     */
                     const void* records, uint32_t n_cap,   /* optional -> layer_*[]               */
                     uint32_t flags, bt_tally* out, void* stream);

/* ---- fan-out of a batch to K queues by RSS flow hash ---------------------------------
 * What a capture pipeline does next with the packets that passed: hand each one to one of K
 * workers so that a flow stays on one worker (the reference's ThreadPool / PluginManager
 * shards, PACKET_FANOUT_HASH on ingest), for a batch that stays on the device. The hash is the
 * Microsoft RSS Toeplitz hash (MSB first) of the flow key under a 40-byte key, and
 * queue = reta[hash & 127], so a host can reproduce its NIC's queue choice.
 * The flow key is defined on the bt_rec the parser gives for the frame (the layer walk and its
 * ok bits, so tagged, QinQ and IP-option frames key on their real addresses and ports):
 *   ok & BT_L_IPV4: source_ip | destination_ip (BT_FLOW_V4), followed by source_port |
 *     destination_port in wire order when ok & (BT_L_TCP | BT_L_UDP) and
 *     (ipv4.flags & 0x3FFF) == 0, neither MF nor a fragment offset (BT_FLOW_V4_L4): every
 *     fragment of a datagram lands in one queue;
 *   ok & BT_L_IPV6: the 32 address bytes (BT_FLOW_V6), plus the ports when TCP or UDP parsed
 *     (BT_FLOW_V6_L4); no extension-header walk, as in the parser;
 *   ICMP never adds ports, BT_FANOUT_L3_ONLY never hashes ports; anything else is
 *   BT_FLOW_NONE with hash 0.
 * `select` has the verdict-word layout (out->verdict of a filter call is one; NULL = all n);
 * bits at or above n are ignored. Both descriptor formats and fixed stride (frame length
 * min(stride, 65535) in bytes[]) are taken. Frame bytes are read under the rule of
 * bt_parse_filter_device: no load outside the 16-B granules of [base, base + bytes), bytes past
 * `bytes` read as zeros, so the key equals the one from that call's record.
 * Asynchronous on `stream` (NULL = the context's stream), no host synchronisation, three kernel
 * launches (two without out->idx; none for n == 0, which still writes *result on the stream), no global atomics: every
 * output is bit-identical from run to run. No allocation once bt_reserve(n) has been called.
 * Nothing is written at or past n_selected in idx, past n in hash / queue, or past
 * queues * ceil(n / 64) words in select_q.
 * BT_E_INVALID_ARGUMENT: a null context, frames, opts, out or result (or a result that is not
 * 8-byte aligned), BT_BATCH_PREFIXES / BT_BATCH_LEAN, a batch bt_parse_filter_device refuses,
 * queues outside 1..64, a reta entry >= queues, both key flags, unknown flag bits. */
#define BT_FANOUT_MAX_QUEUES 64u
#define BT_FANOUT_KEY_USER      0x1u  /* use opts->key; else the RSS verification key (6d5a56da 255b0ec2 ... 6a42b73b beac01fa) */
#define BT_FANOUT_KEY_SYMMETRIC 0x2u  /* the 0x6d5a-repeated key; exclusive with KEY_USER */
#define BT_FANOUT_RETA_USER     0x4u  /* use opts->reta (every entry < queues); else reta[i] = i % queues */
#define BT_FANOUT_L3_ONLY       0x8u  /* never hash ports */
typedef struct bt_fanout_opts { uint32_t queues /*1..64*/, flags; uint8_t key[40]; uint8_t reta[128]; } bt_fanout_opts;

enum { BT_FLOW_NONE = 0, BT_FLOW_V4 = 1, BT_FLOW_V4_L4 = 2, BT_FLOW_V6 = 3, BT_FLOW_V6_L4 = 4 };
typedef struct bt_fanout_result {      /* 808 B, device-visible, 8-byte aligned */
    uint32_t n, n_selected;
    uint32_t start[65];                /* queue q = idx[start[q] .. start[q+1]); start[queues..64] = n_selected */
    uint32_t pad0;
    uint64_t bytes[64];                /* selected frames' lengths per queue (min(len, 65535), as the pack) */
    uint32_t klass[5];                 /* selected packets by BT_FLOW_* */
    uint32_t pad1;
} bt_fanout_result;
typedef struct bt_fanout_out {         /* device-visible; all but result optional */
    uint32_t* hash;      /* n: the hash of every packet in [0, n), selected or not (0 for BT_FLOW_NONE) */
    uint8_t*  queue;     /* n: the queue of a selected packet, 0xFF otherwise */
    uint32_t* idx;       /* n entries: the selected packets' indices grouped by queue, ascending inside a queue */
    uint64_t* select_q;  /* queues * ceil(n/64) words: row q is a verdict-layout selection of queue q's packets,
                            usable as-is as bt_pass_pack_device's `select`; bits at or above n are 0 */
    bt_fanout_result* result;
} bt_fanout_out;
int  bt_flow_fanout_device(bt_ctx* ctx, const bt_batch* frames, const uint64_t* select /* NULL = all n */,
                           const bt_fanout_opts* opts, const bt_fanout_out* out, void* stream);
/* Host only, no context: the class, hash and queue of one frame of `len` readable bytes (any
 * output may be NULL). BT_E_INVALID_ARGUMENT: a null frame with len > 0, opts as above. */
int  bt_flow_hash_host(const uint8_t* frame, uint32_t len, const bt_fanout_opts* opts, uint32_t* hash,
                       uint32_t* klass, uint32_t* queue);

/* ---- per-batch flow table: flow ids and flow records -----------------------------------
 * Which flows are in this batch, and how many packets and bytes does each carry (the NetFlow /
 * conntrack view): an exact group-by on the flow key over a device-resident batch. The key and
 * class of a packet are exactly those of bt_flow_fanout_device (the walk, the fragment rule, no
 * IPv6 extension headers, the read rule); two packets are one flow when class and key bytes are
 * equal: keys are compared, never hashes. No Toeplitz key is involved; the table's probe hash
 * is a fixed function of the key bytes and the class.
 * BT_FLOWTAB_BIDIRECTIONAL: endpoint A = source address followed by the source port (no port in
 * the address-only classes), endpoint B the same of the destination, compared as byte strings.
 * A > B: the stored key has the endpoints swapped and the packet counts in packets[1] /
 * bytes[1]; A <= B: in [0].
 * Flows are numbered in order of first appearance: flows[f].first is strictly increasing in f.
 * flow_id[i] is that number or a BT_FLOW_ID_* sentinel. flows[f] is written for f < flow_cap
 * only; n_flows is the whole count. Nothing is written at or past n_written in flows or past n
 * in flow_id.
 * opts->slots is a power of two >= 128 (0 = the smallest such power of two >= 2 n; n <= 2^30
 * then). When the keyed flows do not fit, overflow_packets != 0, every other output of the call
 * is unspecified (but in bounds), and the caller repeats the call with more slots. A table
 * with exactly as many slots as flows succeeds.
 * All scratch is the caller's: bt_flow_table_scratch_bytes(n, slots) bytes of device memory,
 * 256-byte aligned, initialised by the call on the stream; the context's workspace is not used.
 * Asynchronous on `stream` (NULL = the context's stream), no host synchronisation, no
 * allocation; n == 0 launches nothing and still writes *result in stream order. Every output
 * is bit-identical from run to run.
 * BT_E_INVALID_ARGUMENT, decided before the context or any HIP call: a null frames, opts, out
 * or result; a result or scratch that is misaligned (8 / 256 bytes; flows 8, flow_id 4);
 * unknown flag bits; slots not a power of two or below 128; scratch_bytes below the need (or a
 * null scratch with n > 0); flows == NULL with flow_cap != 0; BT_BATCH_PREFIXES /
 * BT_BATCH_LEAN; a batch bt_parse_filter_device refuses; then a null context. */
#define BT_FLOWTAB_L3_ONLY        0x1u   /* as BT_FANOUT_L3_ONLY: never key on ports */
#define BT_FLOWTAB_BIDIRECTIONAL  0x2u   /* both directions of a conversation are one flow */
#define BT_FLOW_ID_UNSELECTED 0xFFFFFFFFu /* packet not in `select` */
#define BT_FLOW_ID_NONE       0xFFFFFFFEu /* selected, BT_FLOW_NONE: no key, not in the table */
#define BT_FLOW_ID_OVERFLOW   0xFFFFFFFDu /* selected, keyed, the table was full */

typedef struct bt_flow_rec {          /* 80 B */
    uint8_t  key[36];    /* as the fan-out's hash input: v4 src(4) dst(4) [sport dport];
                            v6 src(16) dst(16) [sport dport]; wire order; rest zero */
    uint8_t  klass;      /* BT_FLOW_V4 .. BT_FLOW_V6_L4 */
    uint8_t  pad[3];     /* 0 */
    uint32_t first, last;    /* lowest / highest packet index of the flow in the batch */
    uint32_t packets[2];     /* [0] packets in the key's direction, [1] the reverse (BIDIRECTIONAL only, else 0) */
    uint64_t bytes[2];       /* frame lengths, min(len, 65535) as the pack and the fan-out */
    uint64_t reserved;       /* 0 */
} bt_flow_rec;

typedef struct bt_flow_table_opts { uint32_t flags; uint32_t slots; /* 0 = auto */ uint32_t flow_cap; uint32_t reserved; } bt_flow_table_opts;

typedef struct bt_flow_table_result { /* 72 B, device-visible, 8-byte aligned */
    uint32_t n, n_selected, n_flows, n_written;   /* n_written = min(n_flows, flow_cap) */
    uint32_t none_packets, overflow_packets, slots, reserved;
    uint32_t klass_flows[5];  uint32_t pad;        /* flows by class; [BT_FLOW_NONE] = 0 */
    uint64_t none_bytes, keyed_bytes;              /* selected frame lengths without / with a key */
} bt_flow_table_result;

typedef struct bt_flow_table_out {    /* device-visible */
    uint32_t* flow_id;               /* optional, n entries */
    bt_flow_rec* flows;              /* optional when flow_cap == 0; flow_cap entries */
    bt_flow_table_result* result;    /* required */
} bt_flow_table_out;

/* Host only: the scratch a call over n packets with `slots` (0 = auto) needs. */
int  bt_flow_table_scratch_bytes(uint32_t n, uint32_t slots, uint64_t* bytes);
int  bt_flow_table_device(bt_ctx* ctx, const bt_batch* frames, const uint64_t* select /* NULL = all n */,
                          const bt_flow_table_opts* opts, void* scratch, uint64_t scratch_bytes,
                          const bt_flow_table_out* out, void* stream);
/* The same group-by on the calling thread, no context and no device: packed descriptors over
 * base[0 .. bytes), a byte at or past `bytes` reads as zero. flow_id may be NULL. */
int  bt_flow_table_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n,
                        const uint64_t* select, const bt_flow_table_opts* opts, uint32_t* flow_id,
                        bt_flow_rec* flows, bt_flow_table_result* result);

/* ---- flow tracker: a flow table that lives across batches ---------------------------------
 * The per-batch table above forgets everything at the end of a call. The tracker keeps the
 * flows of a whole capture on the device: every batch is merged into a long-lived table by one
 * asynchronous call, flow numbers stay the same from batch to batch, and a second call ages idle
 * flows out and exports their records.
 * The state is one block of the caller's memory, 256-byte aligned, in three parts
 * (bt_flow_track_layout gives their offsets and the block's size, as a bt_flow_track_sizes):
 *   a bt_flow_track_hdr (128 B);
 *   flow_cap records bt_flow_track_rec, dense: record f is flow number f, records at or past
 *     n_flows are zero;
 *   `slots` u32 slot words (open addressing: empty, or a flow number). Private: their content is
 *     not part of the interface and differs between the device and the host form.
 * slots == 0 resolves to the smallest power of two >= max(128, 2 flow_cap); otherwise it is a
 * power of two >= max(128, flow_cap): a table loaded to 1.0 is legal. flow_cap is 1 .. 2^31
 * (slots is a u32; flow numbers stay far below BT_FLOW_ID_EXPIRED), and <= 2^30 with slots == 0.
 * flags: BT_FLOWTAB_L3_ONLY, BT_FLOWTAB_BIDIRECTIONAL, fixed for the life of the state.
 *
 * bt_flow_track_update_device: the batch's flows are those of bt_flow_table_device under the
 * state's flags, in that order (its kernels run unchanged into the scratch). A flow whose (class,
 * key) is in the table is added to its record: packets and bytes per direction, last_batch, last
 * and last_ts = the timestamp of the flow's last packet of the batch in packet order (not the
 * maximum). The other flows are new: the r-th new flow in batch order gets number n_flows + r
 * when that is below flow_cap, with first_ts = the timestamp of its first packet; otherwise it is
 * not inserted, counts in overflow_flows, its packets count in overflow_packets and read
 * BT_FLOW_ID_OVERFLOW in flow_id. A packet's timestamp is upd->ts[i] (device, n entries, any
 * unit) or, with ts == NULL, upd->batch_ts. flow_id[i] is the flow's number in the state or
 * BT_FLOW_ID_UNSELECTED / _NONE / _OVERFLOW. The batch sequence number (hdr.seq, the number of
 * accepted update calls; a record's first_batch / last_batch; it wraps at 2^32) advances on
 * every accepted call, n == 0 included. Every output is exact and bit-identical from run to run
 * (DESIGN.md §4.2e).
 * bt_flow_track_expire_device: a flow is idle when last_ts <= now && now - last_ts > idle. Idle
 * flows are removed in ascending flow number and written to expired[0 .. n_expired); with
 * expired != NULL at most expired_cap of them are removed per call and the others stay (nothing
 * is lost), with expired == NULL every idle flow is dropped. The flows that stay keep their order
 * and are renumbered densely; remap[old] (optional, written for old < n_flows_before) is the new
 * number or BT_FLOW_ID_EXPIRED. A removed key that appears again is a new flow at the end.
 * Both calls are asynchronous on `stream` (NULL = the context's), allocate nothing, never
 * synchronise and never read the device: n_flows lives in the state only. That is why the
 * library remembers flags, flow_cap and slots of every state bt_flow_track_init_device has
 * initialised in this process, by address, and the later calls take them from there. The table
 * holds 256 states: initialising an address again replaces its entry, bt_flow_track_forget(state)
 * (host only; call it before the memory is freed or reused) frees one, and with 256 other states
 * known bt_flow_track_init_device returns BT_E_RESOURCE and launches nothing: no live tracker is
 * ever dropped. A state is known once its init launch has been enqueued. The kernels compare the
 * remembered values with the state's header; when that is not this tracker's (overwritten, or
 * initialised on another stream that has not run yet) they leave the state as it is, report
 * result->status = 1 with every count 0, and an update fills flow_id[0 .. n) with
 * BT_FLOW_ID_UNSELECTED, so that no per-batch number can pass for a number in the state.
 * All scratch is the caller's device memory, 256-byte aligned: bt_flow_track_scratch_bytes(n) for
 * an update of n packets (the per-batch table's scratch at auto slots, n bt_flow_rec, its result,
 * the local-to-global map and the partials; n <= 2^30), bt_flow_track_expire_scratch_bytes(
 * flow_cap) for an expire. Calls on one state must be ordered by the caller (one stream).
 * The host forms do the same over the same layout in host memory, header and records
 * bit-identical to the device's; they read flags, flow_cap and slots from the header.
 * BT_E_INVALID_ARGUMENT, decided before the context or any HIP call: null or misaligned
 * arguments (state and scratch 256 bytes, result / ts / expired 8, flow_id / remap 4); a state
 * that is not an initialised tracker (device: unknown to this process; host: the header's magic,
 * or state_bytes below the header's layout); state_bytes below the layout (init); opts the layout
 * refuses; scratch_bytes below the need; BT_BATCH_PREFIXES / BT_BATCH_LEAN; a batch
 * bt_parse_filter_device refuses; n above 2^30; expired == NULL with expired_cap != 0; then a
 * null context. */
#define BT_FLOW_ID_EXPIRED    0xFFFFFFFBu /* remap[]: the flow was removed by this expire call */
#define BT_FLOW_TRACK_MAGIC   0x4B525446u /* "FTRK" */

typedef struct bt_flow_track_rec {    /* 104 B, 8-byte aligned */
    uint8_t  key[36];    /* as bt_flow_rec */
    uint8_t  klass;
    uint8_t  pad[3];     /* 0 */
    uint32_t first_batch, last_batch;   /* sequence numbers of the update calls */
    uint32_t first, last;               /* packet index inside that batch */
    uint64_t packets[2];
    uint64_t bytes[2];
    uint64_t first_ts, last_ts;
} bt_flow_track_rec;

typedef struct bt_flow_track_hdr {    /* 128 B, at the state's start */
    uint32_t magic, flags, flow_cap, slots;
    uint32_t n_flows, seq;             /* live flows; accepted update calls so far */
    /* running totals over every update call */
    uint64_t selected_packets, keyed_packets, none_packets, overflow_packets;   /* overflow is part of keyed */
    uint64_t selected_bytes, keyed_bytes, none_bytes, overflow_bytes;
    uint64_t reserved[5];
} bt_flow_track_hdr;

typedef struct bt_flow_track_opts { uint32_t flags, flow_cap, slots /* 0 = auto */, reserved; } bt_flow_track_opts;
typedef struct bt_flow_track_sizes { uint64_t total, header, records, slot_words; uint32_t slots, reserved; } bt_flow_track_sizes;
typedef struct bt_flow_track_update { const uint64_t* ts; /* optional, device, n entries */ uint64_t batch_ts; } bt_flow_track_update;

typedef struct bt_flow_track_result { /* 64 B, device-visible, 8-byte aligned */
    uint32_t n, n_selected, none_packets, batch_flows;
    uint32_t new_flows, overflow_flows, overflow_packets, n_flows;   /* n_flows after the call */
    uint32_t seq, status;             /* this batch's sequence number; 0, or 1: not this tracker's state, nothing done */
    uint64_t keyed_bytes, none_bytes, overflow_bytes;
} bt_flow_track_result;
typedef struct bt_flow_track_out { uint32_t* flow_id; /* optional, n */ bt_flow_track_result* result; } bt_flow_track_out;

typedef struct bt_flow_track_expire_result { /* 32 B, device-visible, 8-byte aligned */
    uint32_t n_flows_before, n_flows, n_idle, n_expired;
    uint32_t status, reserved[3];
} bt_flow_track_expire_result;
typedef struct bt_flow_track_expire_out {
    bt_flow_track_rec* expired;      /* optional, expired_cap entries */
    uint32_t expired_cap, reserved;
    uint32_t* remap;                 /* optional, flow_cap entries */
    bt_flow_track_expire_result* result;
} bt_flow_track_expire_out;

/* Host only. */
int  bt_flow_track_layout(uint32_t flow_cap, uint32_t slots, bt_flow_track_sizes* layout);
int  bt_flow_track_scratch_bytes(uint32_t n, uint64_t* bytes);
int  bt_flow_track_expire_scratch_bytes(uint32_t flow_cap, uint64_t* bytes);
int  bt_flow_track_init_device(bt_ctx* ctx, void* state, uint64_t state_bytes, const bt_flow_track_opts* opts, void* stream);
int  bt_flow_track_forget(void* state);   /* host only: BT_E_INVALID_ARGUMENT for a state the process does not know */
int  bt_flow_track_update_device(bt_ctx* ctx, void* state, const bt_batch* frames, const uint64_t* select /* NULL = all n */,
                                 const bt_flow_track_update* upd, void* scratch, uint64_t scratch_bytes,
                                 const bt_flow_track_out* out, void* stream);
int  bt_flow_track_expire_device(bt_ctx* ctx, void* state, uint64_t now, uint64_t idle, void* scratch, uint64_t scratch_bytes,
                                 const bt_flow_track_expire_out* out, void* stream);
/* The same on the calling thread over a state in host memory; packed descriptors as bt_flow_table_host. */
int  bt_flow_track_init_host(void* state, uint64_t state_bytes, const bt_flow_track_opts* opts);
int  bt_flow_track_update_host(void* state, uint64_t state_bytes, const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc,
                               uint32_t n, const uint64_t* select, const bt_flow_track_update* upd /* ts: host */,
                               uint32_t* flow_id, bt_flow_track_result* result);
int  bt_flow_track_expire_host(void* state, uint64_t state_bytes, uint64_t now, uint64_t idle,
                               const bt_flow_track_expire_out* out);

/* ---- per-flow TCP side table: flag unions, connection state, expiry on close ---------------
 * What happened on a flow's connection (NetFlow v5 tcp_flags / IPFIX 6, per direction) beside
 * the flow records above. The table is flow_cap records bt_flow_tcp_rec of the caller's memory;
 * record f belongs to flow number f of a per-batch table or of a tracker. The caller zeroes it
 * once (all-zero = nothing seen); there is no init call.
 * bt_flow_tcp_update_device: packet i contributes when flow_id[i] < flow_cap, the record
 * bt_parse_filter_device gives for its frame has ok & BT_L_TCP, and, for IPv4,
 * (ipv4.flags & 0x3FFF) == 0 (the rule under which the flow key takes ports; independent of
 * BT_FLOWTAB_L3_ONLY). The layers are walked as bt_flow_fanout_device walks them, frame bytes
 * under its read rule. A contributing packet's value is that record's tcp.flags (byte 13 of the
 * TCP header): it is ORed into flags[dir] and counts in syn_packets (SYN set and ACK clear),
 * fin_packets, rst_packets by its bits. dir is the flow table's direction of the packet: 0
 * without BT_FLOWTAB_BIDIRECTIONAL; with it 1 when the key the table forms under table_flags has
 * its endpoints swapped. A flow_id that is a BT_FLOW_ID_* sentinel contributes nothing; any
 * other id >= flow_cap counts in bad_ids and contributes nothing. Nothing is written outside
 * tcp[0 .. flow_cap) and *result.
 * flow_id (device, n entries) comes from bt_flow_table_device or bt_flow_track_update_device
 * under the same table_flags; the caller enqueues this call behind that one and before any
 * expire of the tracker, on one stream. Asynchronous on `stream` (NULL = the context's), no
 * allocation, no host synchronisation; n == 0 still writes *result in stream order. Every output
 * is an OR or an integer sum (counters mod 2^32): bit-identical from run to run.
 * bt_flow_tcp_update_host: the same on the calling thread, bit-identical; packed descriptors over
 * base[0 .. bytes), a byte at or past `bytes` reads as zero.
 * bt_flow_tcp_state: host only and pure. It is a function of the two flag unions, not a
 * sequence-checked state machine: order-free, hence exact when packets are taken in parallel.
 * With u = flags_fwd | flags_rev and bidir = table_flags & BT_FLOWTAB_BIDIRECTIONAL, in this order:
 *   u == 0: BT_TCP_NONE; u & RST: BT_TCP_RESET; FIN in both directions (without bidir: FIN in
 *   flags_fwd): BT_TCP_CLOSED; u & FIN: BT_TCP_CLOSING; no SYN in u: BT_TCP_MIDSTREAM; SYN in
 *   both directions (without bidir: SYN and ACK in flags_fwd): BT_TCP_ESTABLISHED; otherwise
 *   BT_TCP_OPENING.
 * bt_flow_track_expire_tcp_device is bt_flow_track_expire_device with one more way to leave, and
 * it carries the side table: a flow leaves when it is idle (last_ts <= now && now - last_ts >
 * idle), or when its state under the tracker's flags is BT_TCP_CLOSED or BT_TCP_RESET and
 * last_ts <= now && now - last_ts > closed_idle. n_idle counts that predicate; the order, the
 * expired_cap truncation, remap, the dense renumbering and status are the plain expire's. x->tcp
 * (flow_cap records, required) moves with the records: survivor `old` lands at tcp[remap[old]],
 * entries from the new n_flows up to n_flows_before become zero, entries at or past
 * n_flows_before are not touched; x->expired_tcp[k] (optional, expired_cap records, needs
 * out->expired) belongs to expired[k]. Scratch: bt_flow_track_expire_tcp_scratch_bytes(flow_cap),
 * the plain expire's plus flow_cap side records.
 * BT_E_INVALID_ARGUMENT, decided before the context or any HIP call: a null frames, flow_id (with
 * n > 0), tcp (with flow_cap > 0), result or x; misalignment (tcp, expired_tcp and flow_id 4
 * bytes, result 8); unknown flag bits; expired_tcp without out->expired; BT_BATCH_PREFIXES /
 * BT_BATCH_LEAN; a batch bt_parse_filter_device refuses; what the plain expire refuses; then a
 * null context. */
#define BT_TCPF_FIN 0x01u   /* the wire bits of TCP byte 13 */
#define BT_TCPF_SYN 0x02u
#define BT_TCPF_RST 0x04u
#define BT_TCPF_PSH 0x08u
#define BT_TCPF_ACK 0x10u
enum { BT_TCP_NONE = 0, BT_TCP_OPENING = 1, BT_TCP_ESTABLISHED = 2, BT_TCP_CLOSING = 3,
       BT_TCP_CLOSED = 4, BT_TCP_RESET = 5, BT_TCP_MIDSTREAM = 6 };

typedef struct bt_flow_tcp_rec {      /* 16 B, 4-byte aligned; all-zero = nothing seen */
    uint8_t  flags[2];                /* OR of the TCP flags byte, per direction as packets[] of the flow record */
    uint8_t  pad[2];                  /* 0 */
    uint32_t syn_packets;             /* SYN set and ACK clear; mod 2^32 */
    uint32_t fin_packets, rst_packets;
} bt_flow_tcp_rec;

typedef struct bt_flow_tcp_result {   /* 32 B, device-visible, 8-byte aligned */
    uint32_t n, tcp_packets, syn_packets, fin_packets, rst_packets, bad_ids, reserved[2];
} bt_flow_tcp_result;

typedef struct bt_flow_track_expire_tcp {   /* 24 B */
    bt_flow_tcp_rec* tcp;          /* required: the state's side table, flow_cap records */
    bt_flow_tcp_rec* expired_tcp;  /* optional, expired_cap records; needs out->expired */
    uint64_t closed_idle;          /* a CLOSED or RESET flow leaves once now - last_ts > closed_idle */
} bt_flow_track_expire_tcp;

int  bt_flow_tcp_update_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                               uint32_t table_flags, bt_flow_tcp_rec* tcp, uint32_t flow_cap,
                               bt_flow_tcp_result* result, void* stream);
int  bt_flow_tcp_update_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n,
                             const uint32_t* flow_id, uint32_t table_flags, bt_flow_tcp_rec* tcp, uint32_t flow_cap,
                             bt_flow_tcp_result* result);
int  bt_flow_tcp_state(uint32_t flags_fwd, uint32_t flags_rev, uint32_t table_flags);   /* BT_TCP_* */
int  bt_flow_track_expire_tcp_scratch_bytes(uint32_t flow_cap, uint64_t* bytes);
int  bt_flow_track_expire_tcp_device(bt_ctx* ctx, void* state, uint64_t now, uint64_t idle, const bt_flow_track_expire_tcp* x,
                                     void* scratch, uint64_t scratch_bytes, const bt_flow_track_expire_out* out, void* stream);
int  bt_flow_track_expire_tcp_host(void* state, uint64_t state_bytes, uint64_t now, uint64_t idle,
                                   const bt_flow_track_expire_tcp* x, const bt_flow_track_expire_out* out);

/* ---- per-flow statistics side table: protocol, sizes, TTL, payload, handshake stamps --------
 * What kind of flow a flow is (IPFIX protocolIdentifier and friends), beside the flow records
 * and the TCP side table. The table is flow_cap records bt_flow_stat_rec of the caller's memory,
 * 8-byte aligned; record f belongs to flow number f of a per-batch table or of a tracker. The
 * caller zeroes it once (all-zero = nothing seen); there is no init call.
 * Every field is an OR, an integer sum or a maximum, so an update is exact and bit-identical from
 * run to run however many packets are taken in parallel. Minima are stored
 * complemented: ttl_min_c, len_min_c and the *_ts_c stamps hold ~x of the smallest x seen, so that
 * zero reads as "none" and a minimum is a maximum of ~x. A timestamp of 2^64 - 1 therefore reads
 * as absent.
 * bt_flow_stat_update_device: packet i contributes when flow_id[i] < flow_cap and the walk of
 * bt_flow_fanout_device (at most two tags, no IPv6 extension headers) finds a whole IPv4 or IPv6
 * header in its frame. A BT_FLOW_ID_* sentinel contributes nothing; any other id >= flow_cap
 * counts in bad_ids and contributes nothing. dir is the TCP side table's: 0 without
 * BT_FLOWTAB_BIDIRECTIONAL, else 1 when the key the table forms under table_flags has its
 * endpoints swapped. A contributing packet adds
 *   seen |= bits << (16 dir), the BT_FSEEN_* bits below; proto_max = max(.., protocol / next header);
 *   ttl_max[dir], ttl_min_c[dir] from the IPv4 TTL / IPv6 hop limit; len_max[dir], len_min_c[dir]
 *   and len_sq[dir] += length^2 from the frame length min(len, 65535), as bytes[] of the flow record;
 *   with a whole TCP / UDP header under the flow key's rule (BT_FSEEN_L4): payload =
 *   max(0, ip_payload - hdr) in signed 32-bit arithmetic, ip_payload = IPv4 total_length - 4 IHL
 *   or the IPv6 payload_length, hdr = 4 (tcp[12] >> 4) for TCP and 8 for UDP (header fields only:
 *   captures may be snapped); payload_bytes[dir] += payload, payload_packets[dir] += payload > 0;
 *   for such a TCP packet with flags byte fl and timestamp t (upd->ts[i], device, or with ts ==
 *   NULL upd->batch_ts, as the tracker's update): SYN set and ACK clear: syn_ts_c[dir] = max(.., ~t);
 *   SYN and ACK set: synack_ts_c[dir]; ACK set, SYN and RST clear: ack_ts_c[dir].
 * Frame bytes are read under the fan-out's read rule: a byte at or past `bytes` reads as zero.
 * Ordering, stream, n == 0 and the refusals are bt_flow_tcp_update_device's, with a null upd and
 * a misaligned ts (8 bytes) refused too, and `stat` 8-byte aligned. Nothing is written outside
 * stat[0 .. flow_cap) and *result.
 * bt_flow_stat_update_host: the same on the calling thread, bit-identical (upd->ts: host memory).
 * bt_flow_stat_rtt: host only and pure; handshake round-trip times from one record's stamps. The
 * initiator d is the direction that has a syn stamp; with both, the earlier wins and a tie goes to
 * 0; with neither, nothing is reported (has_initiator = 0). rtt_server = synack[1 - d] - syn[d],
 * valid when that synack stamp exists and is >= syn[d]; rtt_client = ack[d] - synack[1 - d],
 * valid when rtt_server is, ack[d] exists and is >= synack[1 - d]. Without
 * BT_FLOWTAB_BIDIRECTIONAL every packet has direction 0 and the reverse direction is another
 * flow: no RTT is ever reported there.
 *
 * bt_flow_track_side_move_device carries any side table (records of rec_bytes bytes, a multiple
 * of 4 in 4 .. 256, 4-byte aligned) through an expire, by the expire's own remap. It is enqueued
 * behind the bt_flow_track_expire_device (or _tcp_) call that wrote m->remap and *m->result and
 * reads n_flows_before, n_flows and n_expired from *m->result on the device. For old <
 * n_flows_before: a survivor goes to side[remap[old]]; the k-th BT_FLOW_ID_EXPIRED entry in
 * ascending old goes to expired_side[k] when k < expired_cap (expired_side optional); entries
 * [n_flows, n_flows_before) become zero; entries at or past n_flows_before are not touched; a
 * remap value that is neither EXPIRED nor < n_flows writes nothing; an expire that removed nothing
 * or reported status = 1 moves nothing. Counts above flow_cap are taken as flow_cap. Scratch:
 * bt_flow_track_side_move_scratch_bytes(flow_cap, rec_bytes), 256-byte aligned. Refused with
 * BT_E_INVALID_ARGUMENT before the context or any HIP call: a null m, side (with flow_cap > 0),
 * remap (with flow_cap > 0), result or scratch; misalignment (side, expired_side, remap 4 bytes,
 * result 8, scratch 256); rec_bytes not a multiple of 4 in 4 .. 256; expired_cap != 0 without
 * expired_side; a non-zero reserved; scratch_bytes below the need; then a null context.
 * bt_flow_track_side_move_host: the same on the calling thread, *m->result in host memory. */
enum { BT_FSEEN_TCP = 0x01, BT_FSEEN_UDP = 0x02, BT_FSEEN_ICMP = 0x04 /* IPv4 and protocol 1 */,
       BT_FSEEN_ICMP6 = 0x08 /* IPv6 and next header 58 */, BT_FSEEN_OTHER = 0x10,
       BT_FSEEN_FRAGMENT = 0x20 /* IPv4 with flags & 0x3FFF != 0 */, BT_FSEEN_IP_OPTIONS = 0x40 /* IPv4 with IHL > 5 */,
       BT_FSEEN_VLAN = 0x80 /* at least one tag */, BT_FSEEN_L4 = 0x100 /* a whole TCP / UDP header under the flow key's rule */ };

typedef struct bt_flow_stat_rec {     /* 128 B, 8-byte aligned; all-zero = nothing seen */
    uint32_t seen;                /* OR of BT_FSEEN_* << (16 * dir) */
    uint32_t proto_max;           /* max of the IPv4 protocol / IPv6 next header */
    uint32_t payload_packets[2];  /* packets with L4 payload > 0; mod 2^32 */
    uint32_t ttl_max[2], ttl_min_c[2];   /* IPv4 TTL / IPv6 hop limit; *_c = ~minimum */
    uint32_t len_max[2], len_min_c[2];   /* frame length min(len, 65535), as bytes[] of the flow record */
    uint64_t payload_bytes[2];    /* L4 payload bytes from the header fields; mod 2^64 */
    uint64_t len_sq[2];           /* sum of length^2; mod 2^64 (with packets[] and bytes[]: the variance) */
    uint64_t syn_ts_c[2], synack_ts_c[2], ack_ts_c[2];   /* ~(earliest timestamp), per direction */
} bt_flow_stat_rec;

typedef struct bt_flow_stat_result {  /* 32 B, device-visible, 8-byte aligned */
    uint32_t n, ip_packets, l4_packets, tcp_packets, bad_ids, reserved[3];
} bt_flow_stat_result;

typedef struct bt_flow_stat_rtt_out { /* 32 B */
    uint32_t has_initiator, initiator;   /* initiator: 0 or 1, 0 when has_initiator == 0 */
    uint32_t server_valid, client_valid;
    uint64_t rtt_server, rtt_client;     /* 0 when not valid */
} bt_flow_stat_rtt_out;

typedef struct bt_flow_side_move {
    void* side;                   /* the side table, flow_cap records of rec_bytes */
    void* expired_side;           /* optional, expired_cap records */
    const uint32_t* remap;        /* the expire's, flow_cap entries */
    const bt_flow_track_expire_result* result;   /* the expire's own, device memory */
    uint32_t rec_bytes /* multiple of 4, 4..256 */, flow_cap, expired_cap, reserved;
} bt_flow_side_move;

int  bt_flow_stat_update_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                                uint32_t table_flags, const bt_flow_track_update* upd, bt_flow_stat_rec* stat,
                                uint32_t flow_cap, bt_flow_stat_result* result, void* stream);
int  bt_flow_stat_update_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n,
                              const uint32_t* flow_id, uint32_t table_flags, const bt_flow_track_update* upd /* ts: host */,
                              bt_flow_stat_rec* stat, uint32_t flow_cap, bt_flow_stat_result* result);
int  bt_flow_stat_rtt(const bt_flow_stat_rec* rec, bt_flow_stat_rtt_out* out);   /* host only, pure */
int  bt_flow_track_side_move_scratch_bytes(uint32_t flow_cap, uint32_t rec_bytes, uint64_t* bytes);
int  bt_flow_track_side_move_device(bt_ctx* ctx, const bt_flow_side_move* m, void* scratch, uint64_t scratch_bytes, void* stream);
int  bt_flow_track_side_move_host(const bt_flow_side_move* m);

/* ---- per-flow mark side table: flows marked by a verdict, whole sessions selected -----------
 * The way back from a verdict to the packets of its connection: a filter call's verdict raises a
 * mark on the flows of its passing packets (bt_flow_mark_update_device), and a selection is built
 * from the marks of every packet's flow (bt_flow_mark_select_device), for the pack, the fan-out,
 * the flow table or the tracker. The table is flow_cap records bt_flow_mark_rec of the caller's
 * memory, 8-byte aligned; record f belongs to flow number f of a per-batch table or of a tracker.
 * The caller zeroes it once (all-zero = never hit); there is no init call. Every field is an OR,
 * an integer sum or a maximum (the earliest stamp is stored complemented, as the statistics'
 * stamps: zero reads as none, so a hit at 2^64 - 1 reads as no first hit), so an update is exact
 * and bit-identical from run to run however many packets are taken in parallel.
 * bt_flow_mark_update_device: `hit` has the verdict-word layout (bit i % 64 of word i / 64;
 * out->verdict of a filter call is one; NULL = every packet in [0, n) is a hit; bits at or above
 * n are ignored). flow_id is read for hit packets only. A hit packet i with flow_id[i] < flow_cap
 * adds to record flow_id[i], with t = upd->ts[i] (device, n entries; only hit packets' are read)
 * or upd->batch_ts when ts is NULL:
 *   marks |= upd->mark; hit_packets += 1; hit_bytes += min(len, 65535), the frame length as
 *   bytes[] of the flow record; first_hit_ts_c = max(.., ~t); last_hit_ts = max(.., t).
 * Only lengths are read from `frames` (both descriptor formats and fixed stride, as the pack and
 * the tally take them), never frame bytes, and only those of hit packets with an id below
 * flow_cap. *result: hit_packets = the hit bits in [0, n); marked_packets = the hits that reached
 * a record; unkeyed_hits = the hits whose id is a BT_FLOW_ID_* sentinel; bad_ids = the hits whose
 * id is neither a sentinel nor below flow_cap (ids of packets that are no hit are not looked at);
 * new_marked_flows = the flows whose marks lacked a bit of upd->mark before the call and took a
 * hit in it, exactly. Ordering, stream, n == 0 and the refusals are bt_flow_tcp_update_device's
 * (there is no table_flags), with these refused too: a null upd, upd->mark == 0, a non-zero
 * upd->reserved, a misaligned ts or table (8 bytes). Nothing is written outside
 * mark_table[0 .. flow_cap) and *result.
 * bt_flow_mark_select_device: m(i) is true when flow_id[i] < flow_cap and mark_table[flow_id[i]]
 * .marks & opts->mask is non-zero, or with BT_FLOW_MARK_ALL_BITS equals opts->mask. opts->op
 * combines it with `base` (verdict layout, ceil(n/64) words; optional with BT_FLOW_MARK_SET,
 * where it is not read, required otherwise): SET out = m; AND out = base & m; OR out = base | m;
 * ANDNOT out = base & ~m. out_select is ceil(n/64) words whose bits at or above n are written as
 * 0 whatever base holds there; base == out_select is allowed, in place (any other overlap is
 * not). *result: n_marked = the packets with m true, n_out = the bits set in out_select, bad_ids
 * = the packets in [0, n) whose id is neither a sentinel nor below flow_cap. The marks are read,
 * never written. Asynchronous on `stream` (NULL = the context's), behind the call that wrote
 * flow_id and every update of the table it should see; no allocation, no host synchronisation;
 * n == 0 writes *result in stream order and no word. BT_E_INVALID_ARGUMENT before the context or
 * any HIP call: a null opts, mask == 0, unknown flags, an unknown op, a non-zero reserved; a null
 * flow_id or out_select (with n > 0), mark_table (with flow_cap > 0) or result; misalignment
 * (flow_id 4 bytes; mark_table, base, out_select and result 8); a missing base where the op needs
 * one; then a null context.
 * bt_flow_mark_update_host / bt_flow_mark_select_host: the same on the calling thread, no context
 * and no device, bit-identical; packed descriptors, upd->ts in host memory.
 * Expiring: there is no call of its own. The table goes through bt_flow_track_side_move_device
 * with rec_bytes = 32 behind the expire, as any side table does. */
#define BT_FLOW_MARK_ALL_BITS 0x1u   /* bt_flow_mark_select_opts.flags: every bit of mask, not any */
enum { BT_FLOW_MARK_SET = 0, BT_FLOW_MARK_AND = 1, BT_FLOW_MARK_OR = 2, BT_FLOW_MARK_ANDNOT = 3 };

typedef struct bt_flow_mark_rec {     /* 32 B, 8-byte aligned; all-zero = never hit */
    uint32_t marks;            /* OR of upd->mark over the updates in which a hit packet of the flow took part */
    uint32_t hit_packets;      /* hit packets of the flow; mod 2^32 */
    uint64_t hit_bytes;        /* their frame lengths, min(len, 65535) as bytes[] of the flow record; mod 2^64 */
    uint64_t first_hit_ts_c;   /* ~(earliest hit timestamp): zero reads as none, as the statistics' stamps */
    uint64_t last_hit_ts;      /* latest hit timestamp */
} bt_flow_mark_rec;

typedef struct bt_flow_mark_update {  /* 24 B */
    uint32_t mark, reserved;   /* mark != 0; reserved 0 */
    const uint64_t* ts;        /* optional, n entries (device form: device memory) */
    uint64_t batch_ts;         /* every hit's timestamp when ts is NULL */
} bt_flow_mark_update;

typedef struct bt_flow_mark_result {  /* 32 B, device-visible, 8-byte aligned */
    uint32_t n, hit_packets, marked_packets, unkeyed_hits, bad_ids, new_marked_flows, reserved[2];
} bt_flow_mark_result;

typedef struct bt_flow_mark_select_opts { uint32_t mask, flags, op, reserved; } bt_flow_mark_select_opts;

typedef struct bt_flow_mark_select_result {   /* 32 B, device-visible, 8-byte aligned */
    uint32_t n, n_marked, n_out, bad_ids, reserved[4];
} bt_flow_mark_select_result;

int  bt_flow_mark_update_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                                const uint64_t* hit /* NULL = all n */, const bt_flow_mark_update* upd,
                                bt_flow_mark_rec* mark_table, uint32_t flow_cap, bt_flow_mark_result* result, void* stream);
int  bt_flow_mark_update_host(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* hit,
                              const bt_flow_mark_update* upd /* ts: host */, bt_flow_mark_rec* mark_table, uint32_t flow_cap,
                              bt_flow_mark_result* result);
int  bt_flow_mark_select_device(bt_ctx* ctx, const uint32_t* flow_id /* device, n */, uint32_t n,
                                const bt_flow_mark_rec* mark_table, uint32_t flow_cap, const bt_flow_mark_select_opts* opts,
                                const uint64_t* base, uint64_t* out_select, bt_flow_mark_select_result* result, void* stream);
int  bt_flow_mark_select_host(const uint32_t* flow_id, uint32_t n, const bt_flow_mark_rec* mark_table, uint32_t flow_cap,
                              const bt_flow_mark_select_opts* opts, const uint64_t* base, uint64_t* out_select,
                              bt_flow_mark_select_result* result);

/* ---- per-flow sequence side table: a packet's position inside its flow, a per-flow cut-off ---
 * The one flow primitive that depends on order: every selected packet with a flow number learns
 * how many packets and bytes of its flow came before it, and "the first K packets / the first B
 * bytes of every connection" becomes a selection for the pack, the fan-out or the tracker. The
 * table is flow_cap records bt_flow_seq_rec of the caller's memory, 8-byte aligned; record f
 * belongs to flow number f of a per-batch table or of a tracker. The caller zeroes it once
 * (all-zero = nothing numbered yet); there is no init call.
 * Numbering: packet i is numbered when its bit is set in `select` (verdict-word layout, NULL =
 * every packet in [0, n); bits at or above n are ignored) and flow_id[i] < flow_cap. With f its
 * flow, P and B table[f].packets and .bytes before the call, p(i) the numbered packets j < i of
 * flow f in this batch and b(i) the sum of their min(len, 65535) (the flow records' length rule):
 * before_pk(i) = P + p(i), before_by(i) = B + b(i), mod 2^64. Order within a batch is the packet
 * index; order across batches is the order of the calls on the stream.
 * out->seq[i] = min(before_pk(i), BT_FLOW_SEQ_MAX), out->byte_off[i] = before_by(i); every packet
 * in [0, n) that is not numbered (not selected, a sentinel id, a bad id) gets BT_FLOW_SEQ_NONE /
 * BT_FLOW_SEQ_OFF_NONE. keep(i): i is numbered, and max_packets == 0 or before_pk(i) <
 * max_packets, and max_bytes == 0 or before_by(i) < max_bytes: the packet that crosses the byte
 * limit is still kept, the next one is not; the decision is on the 64-bit values, not on the
 * saturated seq. out->out_select (verdict layout, ceil(n/64) words): bit i = keep(i), or with
 * BT_FLOW_SEQ_KEEP_UNKEYED also "selected and flow_id[i] is a BT_FLOW_ID_* sentinel"; bits at or
 * above n are written as 0; out_select == select is allowed, in place (any other overlap is not).
 * Each of the three outputs is optional. After the call table[f].packets and .bytes have grown by
 * the flow's numbered packets and bytes of this batch, kept or not. Nothing is written outside
 * table[0 .. flow_cap), the requested outputs, the scratch and *result.
 * *result: selected = the select bits in [0, n); numbered, numbered_bytes = the numbered packets
 * and their bytes; unkeyed = the selected packets with a sentinel id; bad_ids = the selected
 * packets whose id is neither a sentinel nor below flow_cap; kept = the bits out_select holds or
 * would hold; kept_bytes = the min(len, 65535) of kept numbered packets; flows = the distinct
 * flows numbered in this call, exactly; new_flows = those whose record had packets == 0 before.
 * Only lengths are read from `frames` (both descriptor formats and fixed stride), never frame
 * bytes, and only those of numbered packets; flow_id is read for selected packets only.
 * Asynchronous on `stream` (NULL = the context's), behind the call that wrote flow_id; no
 * allocation, no host synchronisation; n == 0 writes *result in stream order and nothing else.
 * scratch: bt_flow_seq_scratch_bytes(n, flow_cap) bytes of device memory, 256-byte aligned; the
 * call initialises what it reads. Every output is exact and bit-identical from run to run.
 * BT_E_INVALID_ARGUMENT before the context or any HIP call: a null opts, out or result; unknown
 * flags; a non-zero reserved; a null flow_id or frames (with n > 0) or table (with flow_cap > 0);
 * misalignment (flow_id, seq 4 bytes; table, select, byte_off, out_select, result 8; scratch 256);
 * a scratch that is too small; then a null context.
 * bt_flow_seq_host: the same on the calling thread, no context, no device and no scratch,
 * bit-identical; packed descriptors.
 * Expiring: there is no call of its own. The table goes through bt_flow_track_side_move_device
 * with rec_bytes = 16 behind the expire, as any side table does. */
#define BT_FLOW_SEQ_KEEP_UNKEYED 0x1u          /* opts.flags: a selected packet whose id is a BT_FLOW_ID_* sentinel is kept */
#define BT_FLOW_SEQ_NONE      0xFFFFFFFFu      /* seq[i] of a packet that was not numbered */
#define BT_FLOW_SEQ_MAX       0xFFFFFFFEu      /* seq[i] saturates here */
#define BT_FLOW_SEQ_OFF_NONE  0xFFFFFFFFFFFFFFFFull

typedef struct bt_flow_seq_rec   { uint64_t packets, bytes; } bt_flow_seq_rec;          /* 16 B; all-zero = nothing numbered yet */
typedef struct bt_flow_seq_opts  { uint64_t max_packets, max_bytes; uint32_t flags, reserved[3]; } bt_flow_seq_opts;   /* 32 B; 0 = no limit */
typedef struct bt_flow_seq_out   { uint32_t* seq; uint64_t* byte_off; uint64_t* out_select; } bt_flow_seq_out;         /* each optional */
typedef struct bt_flow_seq_result {            /* 64 B, device-visible, 8-byte aligned */
    uint32_t n, selected, numbered, unkeyed, bad_ids, kept, flows, new_flows;
    uint64_t numbered_bytes, kept_bytes, reserved[2];
} bt_flow_seq_result;

int  bt_flow_seq_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes);       /* host only */
int  bt_flow_seq_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                        const uint64_t* select /* NULL = all n */, const bt_flow_seq_opts* opts, bt_flow_seq_rec* table,
                        uint32_t flow_cap, const bt_flow_seq_out* out, void* scratch, uint64_t scratch_bytes,
                        bt_flow_seq_result* result, void* stream);
int  bt_flow_seq_host(const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id, const uint64_t* select,
                      const bt_flow_seq_opts* opts, bt_flow_seq_rec* table, uint32_t flow_cap, const bt_flow_seq_out* out,
                      bt_flow_seq_result* result);

/* ---- per-flow stream matching: a payload pattern across packet boundaries ------------------
 * The PAYLOAD filter decides a pattern per packet, over the reference's 100-byte window. This
 * primitive decides it per stream: a match may begin in one packet of a flow and end in a later
 * one, in this batch or in an earlier call.
 * The stream of (flow f, direction d) is the concatenation, in packet order within a batch and in
 * call order across batches, of the L4 payloads of its contributing packets. It is arrival order,
 * not TCP sequence order: retransmissions and reordering are not undone (bt_flow_tcpseq_device in
 * front of this call gives a `select` without the retransmits).
 * Packet i contributes when its bit is set in `select` (verdict-word layout, NULL = every packet in
 * [0, n); bits at or above n are ignored), flow_id[i] < flow_cap, the walk of bt_flow_fanout_device
 * finds a whole TCP or UDP header under the flow key's rule (the statistics table's BT_FSEEN_L4
 * rule: protocol 6 or 17, the whole 20 / 8 header bytes in the frame, IPv4 neither MF nor a
 * fragment offset) and its payload length is > 0. With l3 and l4 the offsets of the two headers:
 * the payload starts at l4 + 4 * (tcp[12] >> 4) for TCP and at l4 + 8 for UDP, and ends at
 * min(frame length, l3 + IPv4 total_length), for IPv6 at min(frame length, l3 + 40 +
 * payload_length): Ethernet padding is not part of the stream, a snapped capture contributes what
 * it holds, and an end at or before the start is no payload. The direction d is the TCP side
 * table's under table_flags (0 without BT_FLOWTAB_BIDIRECTIONAL). Frame bytes are read under the
 * fan-out's read rule: a byte at or past `bytes` reads as zero. A BT_FLOW_ID_* sentinel
 * contributes nothing; any other selected id >= flow_cap counts in bad_ids.
 * The pattern is a blob of bt_flow_stream_compile: bt_payload_dfa_compile_ex(expression, 0) where
 * the result is the bit-parallel form with form == 1 (a search) and flags == 0 (no repeatable
 * position, no anchor, no $). Such a pattern has bounded memory: with P positions its state after
 * any byte is a function of the last P - 1 stream bytes, so every piece of every stream is
 * matched on its own behind its T = P - 1 <= 63 preceding bytes. Everything else returns
 * BT_E_NOT_IMPLEMENTED (+, *, {n,}, ^, $, \b, patterns only the DFA takes, the always / never
 * forms); what std::regex rejects returns BT_E_INVALID_ARGUMENT. info: width = the blob's W,
 * positions = P, tail = T, closure = R.
 * out->hit (optional; verdict layout, ceil(n/64) words, bits at or above n zero): bit i is set iff
 * some match of the pattern ends at a stream byte that belongs to packet i's payload, wherever it
 * began in the same flow and direction. hit == select is allowed, in place.
 * table: flow_cap records bt_flow_stream_rec of the caller's memory, 8-byte aligned, zeroed once
 * (all-zero = nothing seen); d[dir] = the matcher's state after the stream's last contributing
 * byte; hit_packets / stream_packets per direction, mod 2^32. It goes through an expire by
 * bt_flow_track_side_move_device with rec_bytes = 32; there is no expire call of its own.
 * *out->result: selected = the select bits in [0, n); stream_packets, stream_bytes = the
 * contributing packets and their payload bytes; hit_packets = the hit bits; unkeyed = the selected
 * packets with a sentinel id; bad_ids as above; new_hit_flows = the flows with a hit in this call
 * whose record had hit_packets[0] == hit_packets[1] == 0 before it, exactly.
 * Asynchronous on `stream` (NULL = the context's), behind the call that wrote flow_id; no
 * allocation, no host synchronisation; n == 0 writes *result in stream order and nothing else.
 * pattern is host memory (checked before any HIP call), pattern_device a device copy of the same
 * pattern_bytes bytes, 8-byte aligned. scratch: bt_flow_stream_scratch_bytes(n, flow_cap) bytes of
 * device memory, 256-byte aligned; the call initialises what it reads. flow_cap <= 2^31. Nothing
 * is written outside table[0 .. flow_cap), out->hit, the scratch and *out->result; every output is
 * exact and bit-identical from run to run.
 * BT_E_INVALID_ARGUMENT before the context or any HIP call: a null frames, out, out->result,
 * pattern or pattern_device; a null flow_id (with n > 0) or table (with flow_cap > 0);
 * misalignment (flow_id 4 bytes; table, select, hit, result, pattern_device 8; scratch 256);
 * unknown table_flags; a non-zero reserved; a BT_BATCH_PREFIXES / BT_BATCH_LEAN batch; flow_cap
 * above 2^31; a blob the predicate refuses (BT_E_NOT_IMPLEMENTED); a scratch that is too small;
 * then a null context.
 * bt_flow_stream_host: the same on the calling thread, no context, no device and no scratch,
 * bit-identical; packed descriptors. */
typedef struct bt_flow_stream_rec {            /* 32 B; all-zero = nothing seen */
    uint64_t d[2];                             /* the matcher's state after the last contributing byte, per direction */
    uint32_t hit_packets[2], stream_packets[2];
} bt_flow_stream_rec;
typedef struct bt_flow_stream_info { uint32_t width, positions, tail, closure; } bt_flow_stream_info;   /* W, P, T = P - 1, R */
typedef struct bt_flow_stream_out { uint64_t* hit; struct bt_flow_stream_result* result; uint64_t reserved[2]; } bt_flow_stream_out;
typedef struct bt_flow_stream_result {         /* 64 B, device-visible, 8-byte aligned */
    uint32_t n, selected, stream_packets, hit_packets, unkeyed, bad_ids;
    uint64_t stream_bytes;
    uint32_t new_hit_flows, reserved[7];
} bt_flow_stream_result;

int  bt_flow_stream_compile(const char* expression, void* blob, uint32_t cap, uint32_t* size,
                            bt_flow_stream_info* info /* optional */);                 /* host only */
int  bt_flow_stream_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes);    /* host only */
int  bt_flow_stream_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                           const uint64_t* select /* NULL = all n */, uint32_t table_flags, const void* pattern /* host */,
                           const void* pattern_device, uint32_t pattern_bytes, bt_flow_stream_rec* table, uint32_t flow_cap,
                           void* scratch, uint64_t scratch_bytes, const bt_flow_stream_out* out, void* stream);
int  bt_flow_stream_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                         const uint64_t* select, uint32_t table_flags, const void* pattern, uint32_t pattern_bytes,
                         bt_flow_stream_rec* table, uint32_t flow_cap, const bt_flow_stream_out* out);

/* ---- per-flow TCP sequence classification: retransmits, gaps, order -----------------------
 * The sequence primitive numbers a flow's packets and the stream matcher concatenates their
 * payloads, both in arrival order. This primitive reads the TCP sequence numbers: every segment
 * of a (flow, direction) is placed in that direction's sequence space and classified against the
 * highest byte seen so far.
 * Packet i participates when its bit is set in `select` (verdict-word layout, NULL = every packet
 * in [0, n); bits at or above n are ignored), flow_id[i] < flow_cap, the walk of
 * bt_flow_fanout_device finds a whole TCP header under the statistics table's BT_FSEEN_L4 rule
 * (protocol 6, the 20 header bytes in the frame, IPv4 neither MF nor a fragment offset) and its
 * sequence length L is > 0. L comes from header fields only, as the statistics table's payload
 * (a snapped capture still advances): plen = max(0, ip_payload - 4 (tcp[12] >> 4)) in signed
 * 32-bit arithmetic, L = plen + SYN + FIN; RST adds nothing. A pure ACK or a zero-length
 * keep-alive has L = 0: it does not participate, its class is BT_TCPSEQ_NONE and its record is
 * untouched. s is the big-endian 32 bits at tcp[4 .. 8); the direction d is the TCP side table's
 * under table_flags (0 without BT_FLOWTAB_BIDIRECTIONAL). Frame bytes are read under the
 * fan-out's read rule: a byte at or past `bytes` reads as zero. A BT_FLOW_ID_* sentinel
 * contributes nothing; any other selected id >= flow_cap counts in bad_ids.
 * The record of (flow, direction) holds have, last_seq (the s of the last participating packet),
 * pos (that packet's unwrapped start, int64) and hi (the highest unwrapped end seen, int64).
 * Packets are taken in packet order within a batch and in call order across batches:
 *   the first packet of a direction: u = 0, class FIRST, hi = L;
 *   otherwise u = pos + (int64)(int32)(s - last_seq), e = u + L; the class against hi, then hi =
 *   max(hi, e):
 *     IN_ORDER  u == hi;
 *     GAP       u > hi: the segment lies ahead of everything seen; gap_bytes += u - hi;
 *     OLD       u < hi and e <= hi: every byte at or below the highest seen; old_bytes += L;
 *     OVERLAP   u < hi < e; old_bytes += hi - u;
 *   after every participating packet pos = u, last_seq = s.
 * Unwrapping is against the previous packet, so the 2^32 wrap is followed for any flow length, as
 * long as consecutive participating packets of a direction lie within 2^31 of each other (a step
 * of exactly 0x80000000 is taken as -2^31). Behaviour is defined while |u| < 2^63, which cannot be
 * left in fewer than 2^32 packets of one direction.
 * OLD means "retransmitted or late": the table keeps no hole list, so a segment that fills a hole
 * behind a GAP is OLD as well. In a direction whose gap_packets is 0 every OLD packet is a certain
 * duplicate. A reused 5-tuple with a new ISN shows as one large GAP or OLD until the tracker's
 * expire zeroes the record.
 * table: flow_cap records bt_flow_tcpseq_rec (128 B, two bt_flow_tcpseq_dir) of the caller's
 * memory, 8-byte aligned, zeroed once (all-zero = nothing seen); counts mod 2^32, bytes mod 2^64.
 * It goes through an expire by bt_flow_track_side_move_device with rec_bytes = 128; there is no
 * expire call of its own.
 * Outputs, each optional: out->cls, n bytes, the class; out->off, n int64, the unwrapped start u
 * (the packet's offset in its direction's sequence space), BT_TCPSEQ_OFF_NONE for a packet that
 * is not classified; out->out_select (verdict layout, ceil(n/64) words) = select & ~OLD: a
 * selected packet that does not participate stays selected, bits at or above n are written as 0,
 * out_select == select is allowed, in place. It is the selection to hand to bt_flow_stream_device
 * so that a retransmit does not enter a stream twice.
 * *out->result: selected = the select bits in [0, n); seq_packets, seq_bytes = the participating
 * packets and the sum of their L; first .. overlap = the packets of each class; old_bytes,
 * gap_bytes as above; unkeyed = the selected packets with a sentinel id; bad_ids as above.
 * Asynchronous on `stream` (NULL = the context's), behind the call that wrote flow_id; no
 * allocation, no host synchronisation; n == 0 writes *result in stream order and nothing else.
 * scratch: bt_flow_tcpseq_scratch_bytes(n, flow_cap) bytes of device memory, 256-byte aligned; the
 * call initialises what it reads. flow_cap <= 2^31. Nothing is written outside table[0 ..
 * flow_cap), the requested outputs, the scratch and *out->result; every output is exact, equal to
 * the host form's and bit-identical from run to run.
 * BT_E_INVALID_ARGUMENT before the context or any HIP call: a null frames, out or out->result; a
 * null flow_id (with n > 0) or table (with flow_cap > 0); misalignment (flow_id 4 bytes; table,
 * select, off, out_select, result 8; scratch 256); unknown table_flags; a non-zero reserved; a
 * BT_BATCH_PREFIXES / BT_BATCH_LEAN batch; flow_cap above 2^31; a scratch that is too small; then
 * a null context.
 * bt_flow_tcpseq_host: the same on the calling thread as a plain loop, which is the definition;
 * no context, no device and no scratch; packed descriptors. */
enum { BT_TCPSEQ_NONE = 0, BT_TCPSEQ_FIRST = 1, BT_TCPSEQ_IN_ORDER = 2, BT_TCPSEQ_GAP = 3, BT_TCPSEQ_OLD = 4,
       BT_TCPSEQ_OVERLAP = 5 };
#define BT_TCPSEQ_OFF_NONE INT64_MIN
typedef struct bt_flow_tcpseq_dir {            /* 64 B; all-zero = nothing seen */
    int64_t  pos, hi;                          /* the last packet's unwrapped start; the highest unwrapped end seen */
    uint32_t last_seq, have;
    uint32_t seq_packets, old_packets, gap_packets, overlap_packets;
    uint64_t old_bytes, gap_bytes, reserved;
} bt_flow_tcpseq_dir;
typedef struct bt_flow_tcpseq_rec { bt_flow_tcpseq_dir d[2]; } bt_flow_tcpseq_rec;   /* 128 B, per direction */
typedef struct bt_flow_tcpseq_out {
    uint8_t* cls; int64_t* off; uint64_t* out_select;
    struct bt_flow_tcpseq_result* result;
    uint64_t reserved[2];
} bt_flow_tcpseq_out;
typedef struct bt_flow_tcpseq_result {         /* 64 B, device-visible, 8-byte aligned */
    uint32_t n, selected, seq_packets, first, in_order, gap, old, overlap, unkeyed, bad_ids;
    uint64_t seq_bytes, old_bytes, gap_bytes;
} bt_flow_tcpseq_result;

int  bt_flow_tcpseq_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes);    /* host only */
int  bt_flow_tcpseq_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                           const uint64_t* select /* NULL = all n */, uint32_t table_flags, bt_flow_tcpseq_rec* table,
                           uint32_t flow_cap, void* scratch, uint64_t scratch_bytes, const bt_flow_tcpseq_out* out, void* stream);
int  bt_flow_tcpseq_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                         const uint64_t* select, uint32_t table_flags, bt_flow_tcpseq_rec* table, uint32_t flow_cap,
                         const bt_flow_tcpseq_out* out);

/* ---- per-flow TCP reassembly: a payload pattern matched in sequence order -------------------
 * bt_flow_stream_device matches a pattern across packet boundaries in arrival order;
 * bt_flow_tcpseq_device places every segment in its direction's unwrapped sequence space. This
 * primitive joins the two: within a call the segments of a (flow, direction) are ordered by
 * sequence position, what overlaps is trimmed, and the pattern is matched over the bytes in that
 * order, with the position carried from call to call.
 * Inputs: those of bt_flow_stream_device, and off: n int64, the `off` output of
 * bt_flow_tcpseq_device for the same batch, flow_id and `select`. Pass the same `select` as to
 * that call, not its out_select: a late segment that fills a hole is wanted here. The pattern is
 * a blob of bt_flow_stream_compile, held to the same predicate.
 * Packet i participates when its bit is set in `select`, flow_id[i] < flow_cap, off[i] !=
 * BT_TCPSEQ_OFF_NONE, the walk finds a whole TCP header (the stream matcher's rule with protocol
 * 6) and its captured payload length plen, by the stream matcher's rule, is > 0. Its data range
 * is [ds, de) with ds = off[i] + SYN (a SYN's or FIN's sequence number carries no byte) and de =
 * ds + plen: a snapped segment contributes what was captured, the rest shows as a hole. Sums of
 * positions wrap as unsigned numbers do and compare as signed ones.
 * The record of (flow, direction) holds d, the matcher's state after the last delivered byte,
 * next, the unwrapped position up to which the stream has been delivered, have, and counters.
 * The reorder window is the call. Per (flow, direction), from the record as the call found it:
 *   1. base = next with have, else -2^30: a new stream's window is centred on its first-arrived
 *      segment, whose off is 0.
 *   2. With have, a segment with de <= next is late: late_packets += 1, late_bytes += plen, and
 *      it is dropped.
 *   3. With have, a segment with ds < next < de is trimmed to start at next; dup_bytes += next - ds.
 *   4. rel = ds' - base. A segment with rel < 0 or rel > 0x7FFE0000 is far: counted in
 *      *result and dropped. plen < 2^17, so rel + len fits in 31 bits.
 *   5. The remaining segments are taken in the order (rel, packet index) against a running end
 *      hi, which starts at 0 with have and at the first segment's rel without.
 *   6. For each: rel > hi is a hole: holes += 1, hole_bytes += rel - hi, and the matcher's state
 *      becomes 0 (no match spans missing bytes). rel + len <= hi is a whole duplicate:
 *      dup_packets += 1, dup_bytes += len, nothing is delivered. Otherwise the bytes [max(rel,
 *      hi), rel + len) are delivered to the matcher, dup_bytes += max(hi - rel, 0) and
 *      stream_packets += 1. Then hi = max(hi, rel + len). Where two segments hold different
 *      bytes for a position, the first in (rel, index) order wins.
 *   7. After the call next = base + hi, have = 1, d = the state after the last delivered byte. A
 *      direction none of whose segments got past 2. - 4. keeps next, have and d.
 *   8. A hole still open at the end of a call is given up: the segment that would have filled it
 *      is late in the next call. This is what bounds the memory to the record.
 * out->hit (optional; verdict layout): bit i is set iff a match ends in a byte delivered from
 * packet i. out->rest (optional): `select` restricted to the packets whose off is
 * BT_TCPSEQ_OFF_NONE (UDP, and whatever the sequence call did not place): the selection to hand
 * to bt_flow_stream_device for an arrival-order match of everything else. Each may be `select`,
 * in place; they may not be one another.
 * table: flow_cap records bt_flow_reasm_rec (128 B, two bt_flow_reasm_dir), 8-byte aligned,
 * zeroed once; counts mod 2^32, bytes mod 2^64. It goes through an expire by
 * bt_flow_track_side_move_device with rec_bytes = 128.
 * *out->result: selected, unkeyed, bad_ids as in the stream family; stream_packets, stream_bytes
 * = the packets that delivered a byte and the bytes delivered; hit_packets = the hit bits;
 * new_hit_flows = the flows with a hit in this call whose record had hit_packets == 0 in both
 * directions before it; holes, dup_packets, late_packets, far_packets as above.
 * Asynchronous on `stream`, no allocation, no host synchronisation; n == 0 writes *result in
 * stream order and nothing else. scratch: bt_flow_reasm_scratch_bytes(n, flow_cap) bytes, 256-byte
 * aligned. Every output is exact, equal to the host form's and bit-identical from run to run.
 * BT_E_INVALID_ARGUMENT before the context or any HIP call, as bt_flow_stream_device, with: a null
 * off (with n > 0); off, rest not 8-byte aligned; hit == rest.
 * bt_flow_reasm_host: the same on the calling thread as a plain loop, which is the definition. */
typedef struct bt_flow_reasm_dir {             /* 64 B; all-zero = nothing seen */
    uint64_t d;                                /* the matcher's state after the last delivered byte */
    int64_t  next;                             /* the unwrapped position up to which the stream has been delivered */
    uint32_t have, stream_packets, hit_packets, holes, dup_packets, late_packets;
    uint64_t dup_bytes, hole_bytes, late_bytes;
} bt_flow_reasm_dir;
typedef struct bt_flow_reasm_rec { bt_flow_reasm_dir d[2]; } bt_flow_reasm_rec;   /* 128 B, per direction */
typedef struct bt_flow_reasm_out {
    uint64_t* hit; uint64_t* rest;
    struct bt_flow_reasm_result* result;
    uint64_t reserved[2];
} bt_flow_reasm_out;
typedef struct bt_flow_reasm_result {          /* 64 B, device-visible, 8-byte aligned */
    uint32_t n, selected, unkeyed, bad_ids, stream_packets, hit_packets, new_hit_flows, holes, dup_packets, late_packets,
             far_packets, reserved0;
    uint64_t stream_bytes, reserved1;
} bt_flow_reasm_result;

int  bt_flow_reasm_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes);     /* host only */
int  bt_flow_reasm_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                          const uint64_t* select /* NULL = all n */, const int64_t* off /* device, n */, uint32_t table_flags,
                          const void* pattern /* host */, const void* pattern_device, uint32_t pattern_bytes,
                          bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                          const bt_flow_reasm_out* out, void* stream);
int  bt_flow_reasm_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                        const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern,
                        uint32_t pattern_bytes, bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out);

/* ---- per-flow TCP reassembly, exported: every stream's delivered bytes in order ---------------
 * bt_flow_reasm_device orders the segments of every (flow, direction), trims what overlaps, cuts
 * at holes, and keeps one hit bit per packet. This call does exactly that call's work on the same
 * bt_flow_reasm_rec table, and also writes the delivered bytes themselves: the reassembly
 * counterpart of bt_pass_pack_device, per-flow in-order byte streams where that call gives packed
 * frames. The arguments before `fo` are those of bt_flow_reasm_device; with a
 * pattern, hit, rest, the table and *out->result are bit-identical to what that call writes from
 * the same inputs. Use one of the two calls per batch on a given table, never both. On top of the
 * rules 1. - 8. above:
 * fo->bytes receives every delivered byte of the call, rule 6.'s [max(rel, hi), rel + len) of
 *   every delivering segment, concatenated in ascending flow << 1 | direction and inside a stream
 *   in rule 5.'s (rel, packet index) order. total = out->result->stream_bytes as a 64-bit count.
 *   A byte whose output position is below fo->cap is written; nothing at or past cap is ever
 *   written and [written, cap) is left untouched; written = min(total, cap). cap >=
 *   frames->bytes always suffices; cap == 0 with bytes == NULL is a size query. A source byte
 *   outside [0, frames->bytes) reads as zero, as in the host form; nothing outside the buffer is
 *   read for the copy.
 * fo->runs: a run is a maximal piece of one direction's stream with no hole inside. A run starts
 *   at a stream's first delivering segment of the call and at every segment with rel > hi. Runs
 *   are numbered in output order, so they ascend by (flow << 1 | direction, pos) and by `at`. Run
 *   k is written iff k < run_cap, with its true `at` and `len` even where they pass cap: the
 *   reader clips. n_runs counts all runs; runs_written = min(n_runs, run_cap). run_cap >= n
 *   always suffices. flags: bit 0 the direction; BT_FOLLOW_NEW: the direction's record had have
 *   == 0 when the call found it (on every run of that direction in the call); BT_FOLLOW_HOLE:
 *   bytes are missing in front of the run (rule 6.'s hole). With neither, the run continues
 *   exactly at the record's previous `next`. pos = base + max(rel, hi) of the run's first
 *   segment: the unwrapped position of its first byte, in off's space.
 * fo->place (optional, n entries): the output offset of packet i's first delivered byte, and
 *   UINT64_MAX for every packet that delivered none (unselected and unplaced ones included).
 * No pattern: pattern == NULL requires pattern_device == NULL and pattern_bytes == 0. No byte is
 *   matched (the match launch is skipped), hit, where given, is written as zeros, hit_packets
 *   and new_hit_flows are 0, and every direction the call advances gets d = 0.
 * BT_E_INVALID_ARGUMENT before the context or any HIP call: everything bt_flow_reasm_device
 *   refuses; a null fo or fo->result; null bytes with cap != 0; null runs with run_cap != 0;
 *   runs, place or result not 8-byte aligned; non-zero reserved fields; [bytes, bytes + cap)
 *   overlapping the frames' buffer; a pattern pointer given without the other, or with
 *   pattern_bytes == 0.
 * Asynchronous on `stream`, no allocation, no host synchronisation; n == 0 writes both results in
 * stream order and nothing else. scratch: bt_flow_follow_scratch_bytes(n, flow_cap) bytes,
 * 256-byte aligned. Every output is exact, equal to the host form's and bit-identical from run to
 * run.
 * bt_flow_follow_host: the same on the calling thread as a plain loop, which is the definition. */
#define BT_FOLLOW_DIR   1u
#define BT_FOLLOW_NEW   2u
#define BT_FOLLOW_HOLE  4u
typedef struct bt_flow_follow_run {            /* 32 B: a maximal piece of one direction's stream with no hole inside */
    uint32_t flow;                             /* the flow id */
    uint32_t flags;                            /* BT_FOLLOW_DIR | BT_FOLLOW_NEW | BT_FOLLOW_HOLE */
    uint64_t at;                               /* offset of its first byte in `bytes` (whether or not it fits below cap) */
    int64_t  pos;                              /* unwrapped position of its first byte, in off's space */
    uint64_t len;                              /* its bytes */
} bt_flow_follow_run;
typedef struct bt_flow_follow_result {         /* 32 B, device-visible, 8-byte aligned */
    uint64_t total, written;
    uint32_t n_runs, runs_written;
    uint64_t reserved;
} bt_flow_follow_result;
typedef struct bt_flow_follow_out {            /* 64 B */
    uint8_t* bytes; uint64_t cap;
    bt_flow_follow_run* runs; uint32_t run_cap, reserved0;
    uint64_t* place;                           /* optional, n entries */
    bt_flow_follow_result* result;
    uint64_t reserved[2];
} bt_flow_follow_out;

int  bt_flow_follow_scratch_bytes(uint32_t n, uint32_t flow_cap, uint64_t* bytes);    /* host only */
int  bt_flow_follow_device(bt_ctx* ctx, const bt_batch* frames, const uint32_t* flow_id /* device, n */,
                           const uint64_t* select /* NULL = all n */, const int64_t* off /* device, n */, uint32_t table_flags,
                           const void* pattern /* host, or NULL */, const void* pattern_device, uint32_t pattern_bytes,
                           bt_flow_reasm_rec* table, uint32_t flow_cap, void* scratch, uint64_t scratch_bytes,
                           const bt_flow_reasm_out* out, const bt_flow_follow_out* fo, void* stream);
int  bt_flow_follow_host(const uint8_t* base, uint64_t bytes, const bt_pkt_desc* desc, uint32_t n, const uint32_t* flow_id,
                         const uint64_t* select, const int64_t* off, uint32_t table_flags, const void* pattern,
                         uint32_t pattern_bytes, bt_flow_reasm_rec* table, uint32_t flow_cap, const bt_flow_reasm_out* out,
                         const bt_flow_follow_out* fo);

/* ---- top-K flows of a tracker: the largest flows by a measure, selected on the device ------
 * bt_flow_track_top_device: the k largest flows of the tracker at `state` by opts->metric,
 * selected, ordered and gathered on the device; only k records need leave it.
 * Value: the value of flow f (0 <= f < n_flows) is a u64 computed from its record,
 *   BT_FLOW_TOP_BYTES bytes[0] + bytes[1], BT_FLOW_TOP_PACKETS packets[0] + packets[1] (both mod
 *   2^64), BT_FLOW_TOP_DURATION last_ts >= first_ts ? last_ts - first_ts : 0, BT_FLOW_TOP_TCP_SYN
 *   tcp[f].syn_packets, BT_FLOW_TOP_TCP_RST tcp[f].rst_packets (`tcp`: the tracker's side table,
 *   flow_cap records). total and top_total are sums of values mod 2^64.
 * Order: value descending, then flow number ascending. The top is the first n_top = min(k,
 *   n_flows) flows in that order, and entry r of every output array belongs to rank r. A
 *   zero-valued flow ranks like any other. Ties at the threshold (the value of the last flow of
 *   the top) therefore go to the lowest flow numbers, the earliest-seen flows. n_ties counts the
 *   flows of the whole table whose value equals the threshold; with n_top == 0 threshold and
 *   n_ties are 0.
 * Bounds: nothing is written at or past n_top in any output array; nothing in the state or in
 *   `tcp` is written at all. k == 0 is legal: *result has n_top = 0, n_flows and total.
 * As the tracker's calls: asynchronous on `stream` (NULL = the context's), no allocation, no host
 *   synchronisation and no device-to-host read; the caller orders it on the state's stream behind
 *   the update (and the bt_flow_tcp_update_device) it wants to see. The state's geometry comes
 *   from what the process remembers of it; the kernels compare it with the header and on a
 *   mismatch write status = 1, every other field of *result 0 and nothing else. The host never
 *   knows n_flows: grids are sized by flow_cap and threads at or past n_flows do nothing. Scratch:
 *   bt_flow_track_top_scratch_bytes(flow_cap, k) bytes of the caller's device memory, 256-byte
 *   aligned (one u64 per flow, the histograms, per-block partials, k candidates). Exact and
 *   bit-identical from run to run: integer sums and ordered scans only.
 * bt_flow_track_top_host: the same on the calling thread over a state in host memory (tcp, the
 *   outputs and *result in host memory), bit-identical.
 * BT_E_INVALID_ARGUMENT, decided before the context or any HIP call: a null state, opts, out,
 *   result or scratch; misalignment (state and scratch 256 bytes; result, top_value and top 8;
 *   top_id, tcp and top_tcp 4); k > BT_FLOW_TOP_MAX_K; an unknown metric or non-zero reserved
 *   fields; a TCP metric or top_tcp with tcp == NULL; a state the process does not know (host
 *   form: the header checks of the tracker's host forms); scratch_bytes below the need (which the
 *   state's flow_cap decides); then a null context. */
#define BT_FLOW_TOP_MAX_K 4096u
enum { BT_FLOW_TOP_BYTES = 0,      /* bytes[0] + bytes[1]                        */
       BT_FLOW_TOP_PACKETS = 1,    /* packets[0] + packets[1]                    */
       BT_FLOW_TOP_DURATION = 2,   /* last_ts >= first_ts ? last_ts - first_ts : 0 */
       BT_FLOW_TOP_TCP_SYN = 3,    /* tcp[f].syn_packets  (needs the side table) */
       BT_FLOW_TOP_TCP_RST = 4 };  /* tcp[f].rst_packets  (needs the side table) */

typedef struct bt_flow_top_opts { uint32_t metric, k, reserved[2]; } bt_flow_top_opts;     /* reserved = 0 */
typedef struct bt_flow_top_result {   /* 48 B, device-visible, 8-byte aligned */
    uint32_t n_flows, n_top;          /* n_top = min(k, n_flows) */
    uint32_t status, metric;          /* status as the tracker's: 1 = not this tracker's state, nothing done */
    uint32_t n_ties, reserved;        /* flows of the whole table whose value == threshold */
    uint64_t threshold;               /* value of the last flow of the top, 0 when n_top == 0 */
    uint64_t total, top_total;        /* sum of the value over all flows / over the top, mod 2^64 */
} bt_flow_top_result;
typedef struct bt_flow_top_out {
    uint32_t*          top_id;     /* optional, k entries: flow numbers                  */
    uint64_t*          top_value;  /* optional, k entries                                */
    bt_flow_track_rec* top;        /* optional, k records                                */
    bt_flow_tcp_rec*   top_tcp;    /* optional, k records; needs `tcp`                   */
    bt_flow_top_result* result;    /* required                                           */
} bt_flow_top_out;

int  bt_flow_track_top_scratch_bytes(uint32_t flow_cap, uint32_t k, uint64_t* bytes);   /* host only */
int  bt_flow_track_top_device(bt_ctx* ctx, const void* state, const bt_flow_top_opts* opts,
                              const bt_flow_tcp_rec* tcp /* optional, flow_cap */, void* scratch, uint64_t scratch_bytes,
                              const bt_flow_top_out* out, void* stream);
int  bt_flow_track_top_host(const void* state, uint64_t state_bytes, const bt_flow_top_opts* opts, const bt_flow_tcp_rec* tcp,
                            const bt_flow_top_out* out);

/* ---- endpoint table of a tracker: the tracker's flows aggregated per host on the device ----
 * bt_flow_track_hosts_device: a second exact group-by, on the address instead of the flow key,
 * over the records of the tracker at `state` (Wireshark's "Endpoints" beside its
 * "Conversations"): one bt_flow_host_rec per distinct address.
 * Contributions: every live flow f < n_flows gives two, c = 2 f + role. Role 0 is the key's first
 *   endpoint, role 1 its second; the address is key bytes 0..3 / 4..7 for BT_FLOW_V4 /
 *   BT_FLOW_V4_L4 (family 4, the other 12 address bytes zero) and key bytes 0..15 / 16..31 for
 *   BT_FLOW_V6 / BT_FLOW_V6_L4 (family 6). Ports are never part of a host. Two contributions are
 *   one host when family and the 16 address bytes are equal: bytes are compared, never hashes.
 *   IPv4 1.2.3.4 and IPv6 0102:0304:: are different hosts.
 * Sums: a role-r contribution of flow f adds the record's packets[r] / bytes[r] to the host's
 *   packets[0] / bytes[0] (sent) and packets[1-r] / bytes[1-r] to its [1] (received), 1 to
 *   flows[r], takes the minimum of first_ts, the maximum of last_ts and the minimum of f into
 *   first_flow. That is right for bidirectional trackers and for unidirectional ones, where
 *   packets[1] is 0 and a destination has only received. A flow whose two addresses are equal
 *   contributes twice to the one host: no special case.
 * With `tcp` (the tracker's side table, flow_cap records): tcp_state[bt_flow_tcp_state(flags[0],
 *   flags[1], the tracker's flags)] += 1 for both contributions (BT_TCP_NONE counts too, so the
 *   seven counts sum to flows[0] + flows[1]); syn_flows[0] += 1 when flags[r] has SYN,
 *   syn_flows[1] += 1 when flags[1-r] has it; syn_packets, fin_packets and rst_packets of the
 *   side record are added (mod 2^32). Without `tcp` all of these are 0 and tcp is never read.
 * Order: hosts are numbered in order of first appearance: a host's number is the rank of its
 *   lowest contribution index among all hosts' lowest contribution indices (the rule of the
 *   per-batch table's flows), so hosts[h].first_flow is non-decreasing in h. hosts[h] is written
 *   for h < host_cap only, endpoint_host[c] for c < 2 n_flows only; nothing is written at or
 *   past those bounds, and nothing in the state or in `tcp` is written at all.
 * Slots: opts->slots is a power of two >= 128; 0 = the smallest such power of two >= 4 flow_cap,
 *   which needs flow_cap <= 2^29. When the hosts do not fit, overflow_endpoints != 0, every other
 *   output but status, n_flows and slots is unspecified (but in bounds), and the caller repeats
 *   the call with more slots. A table with exactly as many slots as hosts succeeds.
 * As the top-K call: asynchronous on `stream` (NULL = the context's), no allocation, no host
 *   synchronisation and no device-to-host read; the state's geometry comes from what the process
 *   remembers of it, and on a header mismatch the kernels write status = 1, every other field of
 *   *result 0 and nothing else. Grids are sized by flow_cap; threads at or past n_flows do
 *   nothing. Scratch: bt_flow_track_hosts_scratch_bytes(flow_cap, slots) bytes of the caller's
 *   device memory, 256-byte aligned, initialised by the call (one word per slot, one per
 *   contribution, per-block partials). Exact and bit-identical from run to run: integer sums,
 *   minima, maxima and ordered scans only.
 * bt_flow_track_hosts_host: the same on the calling thread over a state in host memory (tcp, the
 *   outputs and *result in host memory), bit-identical in every output.
 * BT_E_INVALID_ARGUMENT, decided before the context or any HIP call: a null state, opts, out,
 *   result or scratch; misalignment (state and scratch 256 bytes; result and hosts 8; tcp and
 *   endpoint_host 4); slots not a power of two or below 128, or auto slots with flow_cap above
 *   2^29; non-zero reserved fields; hosts == NULL with host_cap != 0; a state the process does
 *   not know (host form: the header checks of the tracker's host forms), or one of 2^31 flows
 *   (its last contribution index would be the empty slot word); scratch_bytes below the need;
 *   then a null context. */
typedef struct bt_flow_host_rec {      /* 128 B, 8-byte aligned */
    uint8_t  addr[16];                 /* IPv4: 4 bytes in wire order, the rest zero; IPv6: 16 */
    uint8_t  family;                   /* 4 or 6 */
    uint8_t  pad[3];                   /* 0 */
    uint32_t first_flow;               /* lowest flow number that has this host as an endpoint */
    uint32_t flows[2];                 /* flows with the host as the key's first / second endpoint */
    uint64_t packets[2], bytes[2];     /* [0] sent by the host, [1] sent to it */
    uint64_t first_ts, last_ts;        /* min of its flows' first_ts, max of their last_ts */
    uint32_t tcp_state[7];             /* its flows by bt_flow_tcp_state (index BT_TCP_*); 0 without tcp */
    uint32_t syn_flows[2];             /* flows whose flags have SYN in the direction the host sends [0] / receives [1] */
    uint32_t syn_packets, fin_packets, rst_packets;   /* sums of its flows' side records, mod 2^32 */
} bt_flow_host_rec;
typedef struct bt_flow_hosts_opts { uint32_t slots /* 0 = auto */, host_cap, reserved[2]; } bt_flow_hosts_opts;
typedef struct bt_flow_hosts_result {  /* 64 B, device-visible, 8-byte aligned */
    uint32_t n_flows, n_hosts, n_written, status;        /* n_written = min(n_hosts, host_cap); status as the tracker's */
    uint32_t overflow_endpoints, slots, hosts_v4, hosts_v6;
    uint64_t packets_total, bytes_total, reserved[2];    /* sums over the flows, mod 2^64 = sums of packets[0] / bytes[0] over all hosts */
} bt_flow_hosts_result;
typedef struct bt_flow_hosts_out {
    bt_flow_host_rec* hosts;           /* optional when host_cap == 0; host_cap records */
    uint32_t* endpoint_host;           /* optional, 2 * flow_cap entries: [2 f + role] = the host number of flow f's endpoint */
    bt_flow_hosts_result* result;      /* required */
} bt_flow_hosts_out;

int  bt_flow_track_hosts_scratch_bytes(uint32_t flow_cap, uint32_t slots, uint64_t* bytes);   /* host only */
int  bt_flow_track_hosts_device(bt_ctx* ctx, const void* state, const bt_flow_hosts_opts* opts,
                                const bt_flow_tcp_rec* tcp /* optional, flow_cap */, void* scratch, uint64_t scratch_bytes,
                                const bt_flow_hosts_out* out, void* stream);
int  bt_flow_track_hosts_host(const void* state, uint64_t state_bytes, const bt_flow_hosts_opts* opts, const bt_flow_tcp_rec* tcp,
                              const bt_flow_hosts_out* out);

/* ---- pcap capture files ------------------------------------------------------------
 * Classic pcap (24-B global header, 16-B record headers), link type 1 (Ethernet), in all four
 * magics: microsecond (0xa1b2c3d4) or nanosecond (0xa1b23c4d) timestamps, in the reader's
 * byte order or swapped. bt_pcap_index is host only (no context, no device):
 *   desc[i] = BT_DESC(offset of record i's data in the file, incl_len) for the first
 *   min(*n, cap) records (desc == NULL: count only), *n = the whole records of the file.
 * A file that ends inside a record header or inside a record's data is not an error: it is
 * indexed up to its last whole record and info->truncated = 1.
 * BT_E_NOT_IMPLEMENTED: another link type, a pcapng file. BT_E_INVALID_ARGUMENT: a null
 * argument, fewer than 24 bytes, an unknown magic, a record with incl_len > 65535 (a
 * descriptor holds 16 bits of length). */
typedef struct bt_pcap_info {
    uint32_t magic;        /* 0xa1b2c3d4 or 0xa1b23c4d (as the writer wrote it)                 */
    uint32_t swapped;      /* 1: the header fields are in the other byte order                  */
    uint32_t nanosecond;   /* 1: ts_usec holds nanoseconds                                      */
    uint32_t snaplen;
    uint32_t linktype;
    uint32_t truncated;    /* 1: bytes after the last whole record that are no whole record     */
    uint64_t end;          /* file offset just past the last whole record (24 with no records)  */
} bt_pcap_info;
int  bt_pcap_index(const uint8_t* file, uint64_t bytes, bt_pcap_info* info, bt_pkt_desc* desc,
                   uint64_t cap, uint64_t* n);
/* The capture filtered by the context's compiled program: `out` receives a pcap holding the
 * input's 24-B global header, then the 16-B record header and the data of every packet whose
 * decision is BT_DECIDE_PASS, verbatim and in order: byte for byte what a host loop over
 * PacketFilter::applyFilters writing the passing records produces. The file is taken in
 * chunks of whole records (at most the context's host_chunk_bytes and host_chunk_packets,
 * and at most 64 MiB / 1M packets), double-buffered: pinned staging, H2D, the filter-only
 * bt_parse_filter_device, bt_pass_pack_device with lead = 16 over its verdict words, and a
 * D2H copy of exactly the packed bytes. A truncated file is filtered up to its last whole
 * record (result->truncated = 1). out == NULL is the size query (result->out_bytes). An out_cap
 * below the need returns BT_E_INVALID_ARGUMENT with result->out_bytes = the need (what fits in
 * whole chunks has been written). A program with a BT_K_HOST slot (an installed CUSTOM
 * callback, a PAYLOAD regex outside the GPU subset) is refused with BT_E_NOT_IMPLEMENTED
 * before any work: the device alone cannot decide its packets. Synchronous; on an error the
 * call's streams are idle when it returns and the first error is the one reported. */
typedef struct bt_pcap_result {
    uint64_t n_in;         /* whole records of the input                                        */
    uint64_t n_pass, n_reject, n_throw;   /* by decision code; their sum is n_in                 */
    uint64_t out_bytes;    /* bytes of the output pcap (24 + the passing records)               */
    uint32_t truncated;
    uint32_t chunks;       /* chunks the file was taken in                                      */
} bt_pcap_result;
int  bt_pcap_filter(bt_ctx* ctx, const uint8_t* file, uint64_t bytes, uint8_t* out, uint64_t out_cap,
                    bt_pcap_result* result);

/* Pipelined form for a stream of batches. The main kernel runs on `stream` as above
 * (records, decide and verdict are complete in stream order); the ordered compaction
 * (pass_idx, n_pass) runs on the context's own compaction stream once that kernel has
 * finished, and `done_event` (a hipEvent_t, may be NULL) is recorded after it. The next
 * call's main kernel on `stream` does not wait for it, so the compaction of batch i runs
 * beside the parse of batch i + 1. Until done_event completes, the caller must neither
 * read pass_idx / n_pass nor rewrite this call's verdict buffer (the compaction reads
 * it): alternate two output sets. */
int  bt_parse_filter_device_async(bt_ctx* ctx, const bt_batch* batch, const bt_outputs* out, void* stream,
                                  void* done_event);

/* Host batch: borrows base/desc for the call, copies through pinned staging in
 * chunks (H2D, kernels, D2H double-buffered on two streams), fills host outputs,
 * returns when done. Output pointers are host memory (records in bt_rec AoS). Records
 * that lie inside a range registered with bt_host_register on this context are written
 * in place by the D2H copies (no pass through the staging). */
int  bt_parse_filter(bt_ctx* ctx, const uint8_t* base, const bt_pkt_desc* desc, uint32_t n,
                     bt_rec* records, uint64_t* verdict, uint8_t* decide,
                     uint32_t* pass_idx, uint32_t* n_pass);

/* The same over a gather list — one pointer + length per frame, e.g. the buffers of a
 * std::vector<beatrice::Packet> (reference include/beatrice/Packet.hpp:145-211). Only
 * the first min(len, 112) bytes of each frame are staged for the device. */
int  bt_parse_filter_ptrs(bt_ctx* ctx, const uint8_t* const* frames, const uint32_t* lens, uint32_t n,
                          bt_rec* records, uint64_t* verdict, uint8_t* decide,
                          uint32_t* pass_idx, uint32_t* n_pass);
/* The bytes of each frame the two calls above read (and stage) with the context's current
 * program: at most min(len, *bytes) from the frame's start; 48 for filter-only calls (which
 * read and stage bytes 12..43 of it), 112 with
 * records, 176 when the program has a GPU PAYLOAD slot (with_records: whether the call asks
 * for records). A caller may pass, in place of a frame, a copy of that many of its first
 * bytes with the frame's true length (e.g. prefixes packed when the packet arrived). */
int  bt_host_stage_bytes(const bt_ctx* ctx, int with_records, uint32_t* bytes);

/* Zero-copy ingest: page-lock a host range (an AF_XDP UMEM, an RX descriptor ring,
 * an output array) and map it into the device; *dev_alias is the pointer kernels
 * use (it may be passed as bt_batch.base / .desc or as an output). The kernels then
 * read the header windows straight over PCIe: no host gather, no staging copy.
 * Registration is in whole pages, in one table for the process (contexts and groups
 * alike): the pages that hold [host, host + bytes) are registered once; a range inside
 * pages a live registration already holds shares them (a reference, no second lock); a
 * range that shares only some of its pages with a live registration is refused
 * (BT_E_INVALID_ARGUMENT: register page-aligned buffers, or one range covering both), so no
 * page is ever locked twice and no unregister unlocks a page another registration still
 * covers. A range is registered once per context. bt_host_unregister drops the context's
 * reference; the last one waits for the devices that hold an alias, then unlocks. The pages
 * must stay mapped (not freed or unmapped) while registered. */
int  bt_host_register(bt_ctx* ctx, void* host, uint64_t bytes, void** dev_alias);
int  bt_host_unregister(bt_ctx* ctx, void* host);

/* ---- PAYLOAD filters on the GPU ---------------------------------
 * Replaces the per-packet std::regex construction + regex_search of
 * PacketFilter::applyPayloadFilter (src/PacketFilter.cpp:288-321) for the regular
 * subset of libstdc++'s ECMAScript grammar: bt_filter_compile compiles every PAYLOAD
 * expression it can once (BT_K_PAYLOAD slots, up to 16 KiB of tables per program); the
 * rest stay BT_K_HOST: backreferences, lookaheads, \c \u, and by default also \b \B,
 * POSIX bracket classes and DFAs of more than 254 live states, which a context created
 * with BT_OPT_PAYLOAD_EXTENDED compiles for the GPU as well. The compiler itself is in
 * include/beatrice_gpu_bench.h.
 *   bt_payload_dfa_eval  applyPayloadFilter(frame, len) on the host with a compiled slot's
 *                        blob (bt_filter_dfa_pool): the C++ filter's continuation of a
 *                        chain the device handed over */
int  bt_payload_dfa_eval(const void* blob, const uint8_t* frame, uint32_t len);

/* ---- capture-ring ingest: AF_PACKET TPACKET_V3 ---------------
 * Replaces the per-packet recv() + heap copy + queue push of the reference's
 * AF_PacketBackend::packetProcessingLoop (src/AF_PacketBackend.cpp:318-363). A
 * PACKET_RX_RING of n_blocks blocks of block_size bytes (linux/if_packet.h,
 * struct tpacket_req3) is mmap'd once; the kernel fills a block with a chain of
 * tpacket3_hdr frames and flips block_status to TP_STATUS_USER. The walker turns
 * ready blocks into bt_pkt_desc entries whose offsets are relative to the ring base,
 * so the ring itself (registered with bt_host_register, or copied to the device) is
 * the bt_batch.base: the frames are never copied on the host. */
typedef struct bt_tpv3_ring {
    void* base;                    /* host address of the mmap'd ring */
    uint64_t block_size;           /* tpacket_req3.tp_block_size      */
    uint32_t n_blocks;             /* tpacket_req3.tp_block_nr        */
    uint32_t reserved;
} bt_tpv3_ring;

/* Takes the ready blocks first_block, first_block+1, ... (mod n_blocks): at most
 * max_blocks of them, stopping at the first block the kernel still owns or whose
 * packets would overflow `cap` descriptors. Writes one descriptor per frame in ring
 * order, BT_DESC(block * block_size + frame offset + tp_mac, min(tp_snaplen, 65535)),
 * and the counts. Blocks are walked in parallel on ctx's host pool (ctx may be NULL:
 * single-threaded, no GPU needed). A malformed block (a frame chain leaving the block)
 * returns BT_E_INVALID_ARGUMENT and takes nothing. The blocks stay owned by the
 * caller until bt_ring_release_tpv3. */
int  bt_ring_walk_tpv3(bt_ctx* ctx, const bt_tpv3_ring* ring, uint32_t first_block,
                       uint32_t max_blocks, bt_pkt_desc* desc, uint32_t cap,
                       uint32_t* n_desc, uint32_t* n_blocks_taken);
#define BT_PREFIX_SLOT 128u
/* Header-prefix gathers: BT_PREFIX_SLOT bytes of `slots` per taken frame (the slot form,
 * bt_ring_gather_tpv3, is in include/beatrice_gpu_bench.h). A batch over `slots`
 * (registered, or copied to the device) runs with flags = BT_BATCH_PREFIXES.
 * The walk with each frame's header prefix packed: the frames of the k-th taken block (whose first
 * descriptor is j_k) go back to back, each 16-B aligned and taking its prefix length rounded
 * up to 16, from byte j_k * BT_PREFIX_SLOT of `slots` (16-B aligned, BT_PREFIX_SLOT * cap
 * bytes, as above); desc[i] = BT_DESC(offset of frame i's prefix, min(tp_snaplen, 65535)),
 * and ring_desc[i] (optional, cap entries) = frame i's ring descriptor as bt_ring_walk_tpv3
 * writes it, for what reads the whole frame (PAYLOAD / CUSTOM slots, forwarding).
 * A block's packets then sit in consecutive bytes (a 42-B UDP header in 48 B), so the
 * kernels' reads of a tile are one contiguous run over PCIe instead of one 128-B slot per
 * packet. Bytes past a prefix belong to the next frame: the batch flag BT_BATCH_PREFIXES
 * (PAYLOAD slots decided on the host) is required as for the slots. */
int  bt_ring_gather_dense_tpv3(bt_ctx* ctx, const bt_tpv3_ring* ring, uint32_t first_block, uint32_t max_blocks,
                               uint8_t* slots, bt_pkt_desc* desc, bt_pkt_desc* ring_desc, uint32_t cap,
                               uint32_t* n_desc, uint32_t* n_blocks_taken);
/* The same walk for filter-only batches: each frame's bytes 12..43 (the 16-B chunk pair
 * holding what every built-in filter reads, zeros past the frame) packed back to back after a
 * 16-B pad at the block's first slot (j_k * BT_PREFIX_SLOT + 16), 32 B per frame;
 * desc[i] = BT_DESC(offset of frame i's 32 B - 12, min(tp_snaplen, 65535)). Run the batch
 * with flags BT_BATCH_PREFIXES | BT_BATCH_LEAN: a call that asks for records is refused. */
int  bt_ring_gather_lean_tpv3(bt_ctx* ctx, const bt_tpv3_ring* ring, uint32_t first_block, uint32_t max_blocks,
                              uint8_t* slots, bt_pkt_desc* desc, bt_pkt_desc* ring_desc, uint32_t cap,
                              uint32_t* n_desc, uint32_t* n_blocks_taken);
/* Hands `count` blocks starting at first_block back to the kernel (TP_STATUS_KERNEL,
 * release-ordered). Call it once the device has finished reading them. */
int  bt_ring_release_tpv3(const bt_tpv3_ring* ring, uint32_t first_block, uint32_t count);

/* The ring stage in one call: up to n_blocks ready blocks from first_block through the
 * context's filter program, in batches of batch_blocks (0 = 128). Each batch is walked on the
 * host (bt_ring_walk_tpv3; with gather, its frames' bytes 12..43 packed into `slots`,
 * bt_ring_gather_lean_tpv3) while the kernels of the batch before it run, so the host walk
 * and the device's PCIe reads overlap. Writes one descriptor (ring-relative in place; slot-
 * relative for gathered batches) and one decision byte per frame in ring order, and, if
 * given, the verdict words and the pass count; stops early at a block the kernel still owns.
 * The ring, desc (cap entries), decide (cap bytes) and, with gather, slots (cap *
 * BT_PREFIX_SLOT bytes, 16-B aligned) must be registered with the context
 * (bt_host_register). Filter-only: the decision bytes are the product (records: the
 * descriptors + bt_parse_filter_device). Replaces the per-frame recv() loop feeding
 * PacketFilter::applyFilters (reference src/AF_PacketBackend.cpp:318-363). */
typedef struct bt_ring_stage_opts {
    uint32_t batch_blocks;        /* blocks per kernel launch (0 = 128)                     */
    uint32_t gather;              /* 1: pack bytes 12..43 of each frame (lean) before launch;
                                     2: adaptive: a batch is gathered while the device is still
                                     busy with earlier batches, read in place once it caught up */
    uint32_t in_place_every;      /* with gather: every k-th batch read in place (0 = none)  */
    uint32_t in_place_blocks;     /* with gather: the last m blocks of every batch read in
                                     place, the rest gathered (0 = whole batches; overrides
                                     in_place_every)                                         */
} bt_ring_stage_opts;
int  bt_ring_stage_tpv3(bt_ctx* ctx, const bt_tpv3_ring* ring, uint32_t first_block, uint32_t n_blocks,
                        const bt_ring_stage_opts* opts, bt_pkt_desc* desc, uint8_t* slots, uint8_t* decide,
                        uint64_t* verdict, uint32_t cap, uint32_t* n_desc, uint32_t* n_pass);
/* The same with flags and two more arguments; flags = 0 is bt_ring_stage_tpv3 exactly (ring_desc
 * unused). BT_RING_RESUME_PAYLOAD, the two-pass PAYLOAD path: a gathered batch holds bytes 12..43
 * of each frame, so its launch leaves BT_DECIDE_HOST at the program's BT_K_PAYLOAD slots; with the
 * flag, and a program that has such a slot, every gathered batch also gets its frames' ring
 * descriptors in `ring_desc` (cap entries, registered with the context like desc; NULL while
 * gathering is BT_E_INVALID_ARGUMENT) and its launch is followed on the same stream by
 * bt_filter_resume_device over (the ring, ring_desc + the batch's start, its count), so gathered
 * and in-place batches decide alike. The host walk of the next batch overlaps both kernels;
 * batches read in place are unchanged. n_host (optional): the frames whose final code is still
 * BT_DECIDE_HOST (CUSTOM slots and PAYLOAD expressions outside the GPU subset); `verdict` and
 * `n_pass` treat those frames as not passed, the host continues them from decide. */
#define BT_RING_RESUME_PAYLOAD 0x1u
int  bt_ring_stage_tpv3_ex(bt_ctx* ctx, const bt_tpv3_ring* ring, uint32_t first_block, uint32_t n_blocks,
                           const bt_ring_stage_opts* opts, uint32_t flags, bt_pkt_desc* desc,
                           bt_pkt_desc* ring_desc, uint8_t* slots, uint8_t* decide, uint64_t* verdict,
                           uint32_t cap, uint32_t* n_desc, uint32_t* n_pass, uint32_t* n_host);

/* ---- several devices in one process -------------------------------
 * The reference runs one daemon process whose capture threads feed one plugin set
 * (src/BeatriceContext.cpp:215-278, src/PluginManager.cpp:158-188). A group is one
 * context per device (its own streams, pinned staging and host threads). The filter
 * program is compiled once on the host and installed on every member. A host batch is
 * split into contiguous ranges that start on 64-packet boundaries and balance the bytes
 * each member stages (bt_group_split), every member runs its range concurrently, and the
 * outputs land in the caller's arrays exactly as bt_parse_filter / _ptrs write them for
 * the whole batch (pass indices in ascending order). No data crosses devices. */
typedef struct bt_group bt_group;
int      bt_group_create(const int* devices, uint32_t n_devices, const bt_opts* opts, bt_group** out);
void     bt_group_destroy(bt_group* group);
uint32_t bt_group_size(const bt_group* group);
bt_ctx*  bt_group_member(bt_group* group, uint32_t k);   /* member k's context (device k) */
int      bt_group_filter_compile(bt_group* group, const bt_filter_desc* filters, uint32_t n);
int      bt_group_parse_filter(bt_group* group, const uint8_t* base, const bt_pkt_desc* desc, uint32_t n,
                               bt_rec* records, uint64_t* verdict, uint8_t* decide, uint32_t* pass_idx,
                               uint32_t* n_pass);
int      bt_group_parse_filter_ptrs(bt_group* group, const uint8_t* const* frames, const uint32_t* lens, uint32_t n,
                                    bt_rec* records, uint64_t* verdict, uint8_t* decide, uint32_t* pass_idx,
                                    uint32_t* n_pass);
/* bt_host_parallel over the whole group's host threads: fn(user, w, workers) runs once for
 * every w in [0, workers), workers = the members' pool sizes summed (member k's pool, on its
 * NUMA node, takes a contiguous range of w); returns when all have. For host-side work on a
 * batch's results (a filter's decision scan, its FilterResults), so that a group spends its
 * whole budget there rather than member 0's share of it. */
int      bt_group_host_parallel(bt_group* group, void (*fn)(void* user, uint32_t worker, uint32_t workers), void* user);

/* Zero-copy over the group (AF_XDP UMEM, TPACKET_V3 ring, output arrays): page-lock a host
 * range once (portable, mapped) and map it into every member's device; each member reads
 * it through its own alias over its own PCIe link. Whole pages, in the same process-wide
 * table as bt_host_register (shared when another registration holds all of the range's
 * pages, refused when it holds only some). A group's ranges must not overlap. The last
 * reference on the pages waits for every device holding an alias, then unlocks. */
int      bt_group_host_register(bt_group* group, void* host, uint64_t bytes);
int      bt_group_host_unregister(bt_group* group, void* host);
/* bt_parse_filter_device over group-registered host memory, split across the members:
 * `batch` and `out` hold HOST addresses. batch.base / batch.desc and out.records /
 * out.verdict / out.decide must lie in ranges registered with bt_group_host_register;
 * out.pass_idx / out.n_pass are written by the host and may be any host memory. The batch
 * is split on 64-packet tiles by bt_group_cost(mapped) and member k runs its range
 * [lo, hi) with its own alias of every buffer: descriptors from desc + lo (fixed stride:
 * base + lo * stride), records at the range's tile (tiled: + lo / 64 * 6144 bytes, n_cap -
 * lo; BT_OPT_RECORDS_AOS: + lo * 96; plane-major records cannot be split and are
 * refused with more than one member), decisions at + lo, verdict words at + lo / 64. The
 * pass list is built from the verdict words on the members' host threads (out.verdict, or
 * the group's own registered words when the caller asked for none), in ascending order.
 * Synchronous: every output is complete on return. */
int      bt_group_parse_filter_mapped(bt_group* group, const bt_batch* batch, const bt_outputs* out);

/* ---- context helpers ------------------------------------------------------------ */
/* Waits for the context's stream and its compaction stream (bt_parse_filter_device_async). */
int  bt_synchronize(bt_ctx* ctx);
/* Runs fn(user, w, workers) once on each of the context's host threads (w = 0 .. workers-1,
 * the caller is worker 0) and returns when all have: the pool that gathers and drains the
 * host-batch pipeline, lent to host-side post-processing of a batch. */
int  bt_host_parallel(bt_ctx* ctx, void (*fn)(void* user, uint32_t worker, uint32_t workers), void* user);
/* Device memory, copies, streams and timing loops for hosts without a HIP toolchain (tests,
 * benchmarks, ctypes): include/beatrice_gpu_bench.h. */

/* ---- user-defined protocols: ProtocolParser with any ProtocolDefinition -------------
 * Replaces ProtocolParser::parsePacketInternal / extractField / extractValue<T>
 * (src/parser/ProtocolParser.cpp:238-433) for a table registered with registerProtocol
 * (include/parser/ProtocolParser.hpp:63-69) or passed as a ProtocolDefinition: one
 * kernel pass extracts every field of every packet of a batch.
 *   span   = ProtocolDefinition::getTotalLength() (src/parser/FieldDefinition.cpp:31-46),
 *            the largest field end; a packet shorter than span is PACKET_TOO_SHORT with no
 *            field (:244-247), a longer one has every field (each ends within span).
 *   values = the result of extractValue<T> for the field's type (:385-433), as the bits
 *            of T zero-extended to 64: integer types and TIMESTAMP assemble the field's
 *            bytes little-endian (LITTLE) or big-endian (BIG / NETWORK / HOST), byte i
 *            shifted by (8 i) mod the width the shift is done in (32 for types narrower
 *            than 64 bits, 64 otherwise) as x86-64 does, then cut to T; FLOAT32 / FLOAT64
 *            are the raw bits when the length is 4 / 8, else 0; BOOLEAN is byte 0 != 0;
 *            byte-typed fields (BYTES, STRING, MAC/IPV4/IPV6_ADDRESS, CUSTOM) are 0.
 *   image  = the packet's bytes [0, span), from which the host materialises rawHex and
 *            the byte-typed fields of the ParseResult.
 * A BOOLEAN field of length 0 is rejected (BT_E_INVALID_ARGUMENT): the reference reads
 * fieldData[0] of an empty vector there. */
#define BT_FIELD_MAX 64u           /* fields per protocol table                          */
enum bt_field_type {               /* FieldType (include/parser/FieldDefinition.hpp:16-35) */
    BT_FT_UINT8 = 0, BT_FT_UINT16, BT_FT_UINT32, BT_FT_UINT64, BT_FT_INT8, BT_FT_INT16, BT_FT_INT32,
    BT_FT_INT64, BT_FT_FLOAT32, BT_FT_FLOAT64, BT_FT_BYTES, BT_FT_STRING, BT_FT_BOOLEAN, BT_FT_MAC,
    BT_FT_IPV4, BT_FT_IPV6, BT_FT_TIMESTAMP, BT_FT_CUSTOM
};
#define BT_ENDIAN_LITTLE 0u        /* Endianness::LITTLE (:37-42); 1..3 all decode big-endian */

typedef struct bt_field_def {      /* FieldDefinition (:61-82): the parts extraction uses */
    uint64_t offset;
    uint64_t length;
    uint32_t type;                 /* bt_field_type                                       */
    uint32_t endianness;           /* Endianness value                                    */
} bt_field_def;

typedef struct bt_extract_out {    /* device-visible; any pointer may be NULL             */
    uint8_t*  status;              /* n bytes: 0 SUCCESS, 9 PACKET_TOO_SHORT (ParseStatus) */
    uint64_t* values;              /* n_fields x n_cap, field-major: values[f * n_cap + i] */
    uint8_t*  image;               /* n x span bytes: packet i at image + i * span, its
                                      bytes [0, span) when SUCCESS, zeros otherwise        */
    uint32_t  n_cap;               /* values column stride (>= n)                         */
    uint32_t  reserved;
} bt_extract_out;

/* getTotalLength() of a field table (0 for no fields). */
int  bt_proto_span(const bt_field_def* fields, uint32_t n_fields, uint64_t* span);
/* Device-resident extraction, asynchronous on `stream` (NULL = the context's stream);
 * the table is copied into the launch, so it need not outlive the call. */
int  bt_extract_device(bt_ctx* ctx, const bt_batch* batch, const bt_field_def* fields, uint32_t n_fields,
                       const bt_extract_out* out, void* stream);
/* Host gather list in (the buffers of a std::vector<Packet>), host outputs back; waits.
 * status: n bytes; values: n_fields x n, values[f * n + i]; image: n x span bytes. Only the
 * [0, span) prefix of each frame is staged for the device. */
int  bt_extract(bt_ctx* ctx, const uint8_t* const* frames, const uint32_t* lens, uint32_t n,
                const bt_field_def* fields, uint32_t n_fields, uint8_t* status, uint64_t* values,
                uint8_t* image);
/* The same outputs computed on the calling thread, no device: for batches too small to pay
 * for a device round trip (GpuProtocolParser::parsePacket of one packet; ≈ 0.1 ms per
 * bt_extract call). extractValue<T>'s bits exactly as bt_extract_tile decodes them. */
int  bt_extract_host(const uint8_t* const* frames, const uint32_t* lens, uint32_t n, const bt_field_def* fields,
                     uint32_t n_fields, uint8_t* status, uint64_t* values, uint8_t* image);
/* ---- text output --------------------------------------------------------------
 * The text the reference's ParseResult formatters print for every walked layer of
 * records [0, n) (reference src/parser/ParserResult.cpp:214-349; each layer is the
 * ParseResult ProtocolParser::parsePacket(slice, name) returns, wall-clock values 0),
 * each layer's text followed by '\n', packets in order. Replaces a loop of
 * parsePacket(...).toJsonString() etc. (e.g. src/beatrice_cli.cpp:1654-1660).
 * `recs` are host bt_rec (AoS, e.g. from bt_parse_filter or bt_record_gather).
 * out == NULL: size query (*out_len = bytes needed). pkt_off (optional, n + 1
 * entries) receives each packet's start offset and the total. A `cap` below the
 * size returns BT_E_INVALID_ARGUMENT with *out_len set. ctx (optional, may be NULL)
 * lends its host thread pool; no device is used. */
#define BT_FMT_JSON  0u   /* ParseResult::toJsonString          (:214-254) */
#define BT_FMT_XML   1u   /* ParseResult::toXmlString           (:256-298) */
#define BT_FMT_CSV   2u   /* ParseResult::toCsvString           (:300-313) */
#define BT_FMT_HUMAN 3u   /* ParseResult::toHumanReadableString (:315-349) */
int  bt_format_records(bt_ctx* ctx, const bt_rec* recs, uint32_t n, uint32_t format, char* out, uint64_t cap,
                       uint64_t* out_len, uint64_t* pkt_off);
/* The same text in one pass: the records are formatted once, then dest(user, bytes) is called
 * once with the exact size and returns where to put it (NULL only when bytes == 0); the
 * size query plus the call above format everything twice. */
int  bt_format_records_to(bt_ctx* ctx, const bt_rec* recs, uint32_t n, uint32_t format,
                          char* (*dest)(void* user, uint64_t bytes), void* user, uint64_t* out_len,
                          uint64_t* pkt_off);

/* host-side record gather from the device layout (after a D2H copy) */
void bt_record_gather(const void* records, uint32_t n_cap, uint32_t i, bt_rec* out);
/* All n records at once (planes != 0: plane-major), on ctx's host threads (ctx may be
 * NULL); *slabs (optional) gets the total of slabs the device stored. out == NULL with
 * slabs != NULL only counts (reads slab 1 of each record). */
int  bt_record_unpack(bt_ctx* ctx, const void* records, uint32_t n_cap, uint32_t n, uint32_t planes, bt_rec* out,
                      uint64_t* slabs);

#ifdef __cplusplus
}
#endif

#if defined(__cplusplus)
static_assert(sizeof(bt_rec) == BT_REC_BYTES, "bt_rec must be 96 bytes");
static_assert(offsetof(bt_rec, l3) == 28, "L3 union at 28");
static_assert(offsetof(bt_rec, l4) == 68, "L4 union at 68");
static_assert(offsetof(bt_rec, detect_code) == 88, "detector column at 88");
static_assert(sizeof(bt_tally) == 2304 && offsetof(bt_tally, code) == 40, "bt_tally is 2,304 bytes");
#endif

#endif /* BEATRICE_GPU_H */
