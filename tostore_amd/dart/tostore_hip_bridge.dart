// tostore_hip_bridge.dart -- the `dart:ffi` binding a ToStore maintainer adds as
// lib/src/handler/hip_vector_backend.dart to route vectorSearch() through
// libtostore_hip.so (include/tostore_hip.h).
//
// NOT compiled in this repository: the build image has no Dart SDK.  What CAN be
// checked without one is: tests/test_dart_bridge.py parses every `typedef ...C`
// below, the symbol each one is looked up as, and the TshNghInfo / TshCounters
// structs, and compares arity, argument widths and field layout with
// include/tostore_hip.h; a header symbol that is neither bound here nor on that
// test's short "not for a Dart host" list fails the test.
// It is a mechanical mapping of the C-ABI, written in the style of the
// reference's only existing FFI user, lib/src/handler/system_ffi_helper.dart
// (DynamicLibrary.open + lookupFunction, int32 status with 0 = success,
// calloc/free in try/finally, every failure falls back to the Dart path).
// The ctypes binding tostore_amd/_ffi.py exercises the same entry points with
// the same argument meaning and IS tested (tests/test_abi.py, tests/test_gpu_*).

import 'dart:async';
import 'dart:ffi';
import 'dart:math' show Random;
import 'dart:typed_data';

import 'package:ffi/ffi.dart';

import '../core/ngh_graph_engine.dart' show NghSearchResult;
import '../core/vector_quantizer.dart' show PqCodebook;
import '../model/ngh_index_meta.dart';
import '../model/table_schema.dart' show VectorDistanceMetric;
import 'logger.dart';

// ---- native signatures (include/tostore_hip.h) ---------------------------------
typedef _AbiVersionC = Int32 Function();
typedef _AbiVersionD = int Function();
typedef _DeviceCountC = Int32 Function();
typedef _DeviceCountD = int Function();
typedef _LastErrorC = Int32 Function(Pointer<Utf8>, Int32);
typedef _LastErrorD = int Function(Pointer<Utf8>, int);
typedef _CreateC = Int32 Function(Int32, Int32, Int64, Int32, Pointer<Pointer<Void>>);
typedef _CreateD = int Function(int, int, int, int, Pointer<Pointer<Void>>);
typedef _DestroyC = Int32 Function(Pointer<Void>);
typedef _DestroyD = int Function(Pointer<Void>);
typedef _AppendC = Int32 Function(Pointer<Void>, Int64, Int64, Pointer<Float>);
typedef _AppendD = int Function(Pointer<Void>, int, int, Pointer<Float>);
typedef _SetDeletedC = Int32 Function(Pointer<Void>, Pointer<Int64>, Int64);
typedef _SetDeletedD = int Function(Pointer<Void>, Pointer<Int64>, int);
typedef _LoadRawvecC = Int32 Function(
    Pointer<Void>, Pointer<Utf8>, Int32, Int32, Int64, Int64, Pointer<Int64>);
typedef _LoadRawvecD = int Function(
    Pointer<Void>, Pointer<Utf8>, int, int, int, int, Pointer<Int64>);
typedef _SizeC = Int64 Function(Pointer<Void>);
typedef _SizeD = int Function(Pointer<Void>);
typedef _SearchC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Double,
    Pointer<Uint8>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchD = int Function(Pointer<Void>, Pointer<Float>, int, int, double,
    Pointer<Uint8>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _OpenNghC = Int32 Function(
    Pointer<Utf8>, Int32, Int32, Pointer<Pointer<Void>>, Pointer<TshNghInfo>);
typedef _OpenNghD = int Function(
    Pointer<Utf8>, int, int, Pointer<Pointer<Void>>, Pointer<TshNghInfo>);
typedef _OpenNghShardC = Int32 Function(
    Pointer<Utf8>, Int32, Int32, Int32, Int32, Pointer<Pointer<Void>>, Pointer<TshNghInfo>);
typedef _OpenNghShardD = int Function(
    Pointer<Utf8>, int, int, int, int, Pointer<Pointer<Void>>, Pointer<TshNghInfo>);
typedef _MaskCreateC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Int64, Pointer<Pointer<Void>>);
typedef _MaskCreateD = int Function(Pointer<Void>, Pointer<Uint8>, int, Pointer<Pointer<Void>>);
typedef _MaskDestroyC = Int32 Function(Pointer<Void>);
typedef _MaskDestroyD = int Function(Pointer<Void>);
typedef _MaskKeptC = Int64 Function(Pointer<Void>);
typedef _MaskKeptD = int Function(Pointer<Void>);
typedef _AttrCreateC = Int32 Function(Pointer<Void>, Pointer<Int64>, Int64, Pointer<Void>);
typedef _AttrCreateD = int Function(Pointer<Void>, Pointer<Int64>, int, Pointer<Void>);
typedef _AttrSetC = Int32 Function(Pointer<Void>, Int64, Int64, Pointer<Int64>);
typedef _AttrSetD = int Function(Pointer<Void>, int, int, Pointer<Int64>);
typedef _AttrDestroyC = Int32 Function(Pointer<Void>);
typedef _AttrDestroyD = int Function(Pointer<Void>);
typedef _MaskCreateRangeC = Int32 Function(
    Pointer<Void>, Pointer<Void>, Int64, Int64, Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _MaskCreateRangeD = int Function(
    Pointer<Void>, Pointer<Void>, int, int, int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _MaskReadC = Int32 Function(Pointer<Void>, Pointer<Uint8>, Int64);
typedef _MaskReadD = int Function(Pointer<Void>, Pointer<Uint8>, int);
typedef _MaskCreateWhereC = Int32 Function(Pointer<Void>, Pointer<Void>, Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _MaskCreateWhereD = int Function(Pointer<Void>, Pointer<Void>, int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _TagsCreateC = Int32 Function(Pointer<Void>, Pointer<Int64>, Int64, Pointer<Int64>, Pointer<Void>);
typedef _TagsCreateD = int Function(Pointer<Void>, Pointer<Int64>, int, Pointer<Int64>, Pointer<Void>);
typedef _TagsSetC = Int32 Function(Pointer<Void>, Int64, Int64, Pointer<Int64>, Pointer<Int64>);
typedef _TagsSetD = int Function(Pointer<Void>, int, int, Pointer<Int64>, Pointer<Int64>);
typedef _TagsDestroyC = Int32 Function(Pointer<Void>);
typedef _TagsDestroyD = int Function(Pointer<Void>);
typedef _MaskCreateTagsC = Int32 Function(
    Pointer<Void>, Pointer<Void>, Pointer<Int64>, Int64, Int32, Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _MaskCreateTagsD = int Function(
    Pointer<Void>, Pointer<Void>, Pointer<Int64>, int, int, int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _AttrFacetsC = Int32 Function(
    Pointer<Void>, Pointer<Void>, Pointer<Void>, Int32, Pointer<Int64>, Int64, Pointer<Int64>, Pointer<Int64>);
typedef _AttrFacetsD = int Function(
    Pointer<Void>, Pointer<Void>, Pointer<Void>, int, Pointer<Int64>, int, Pointer<Int64>, Pointer<Int64>);
typedef _TagsFacetsC = Int32 Function(
    Pointer<Void>, Pointer<Void>, Pointer<Void>, Pointer<Int64>, Int64, Pointer<Int64>, Pointer<Int64>);
typedef _TagsFacetsD = int Function(
    Pointer<Void>, Pointer<Void>, Pointer<Void>, Pointer<Int64>, int, Pointer<Int64>, Pointer<Int64>);
typedef _SearchMaskedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Double,
    Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchMaskedD = int Function(Pointer<Void>, Pointer<Float>, int, int, double,
    Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SubmitMaskedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Pointer<Void>, Pointer<Int32>);
typedef _SubmitMaskedD = int Function(Pointer<Void>, Pointer<Float>, int, Pointer<Void>, Pointer<Int32>);
typedef _PqEncodeC = Int32 Function(
    Pointer<Void>, Int64, Int64, Pointer<Float>, Int32, Int32, Pointer<Uint8>);
typedef _PqEncodeD = int Function(
    Pointer<Void>, int, int, Pointer<Float>, int, int, Pointer<Uint8>);
typedef _PqTrainC = Int32 Function(Int32, Pointer<Float>, Int64, Int32, Int32, Int32, Int32,
    Pointer<Int32>, Pointer<Float>);
typedef _PqTrainD = int Function(int, Pointer<Float>, int, int, int, int, int,
    Pointer<Int32>, Pointer<Float>);

typedef _CreateShardC = Int32 Function(Int32, Int32, Int64, Int32, Int64, Pointer<Pointer<Void>>);
typedef _CreateShardD = int Function(int, int, int, int, int, Pointer<Pointer<Void>>);
typedef _DimC = Int32 Function(Pointer<Void>);
typedef _DimD = int Function(Pointer<Void>);
typedef _MetricC = Int32 Function(Pointer<Void>);
typedef _MetricD = int Function(Pointer<Void>);
typedef _MaxInflightC = Int32 Function();
typedef _MaxInflightD = int Function();
typedef _SubmitC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Pointer<Uint8>, Pointer<Int32>);
typedef _SubmitD = int Function(Pointer<Void>, Pointer<Float>, int, Pointer<Uint8>, Pointer<Int32>);
typedef _ReadyC = Int32 Function(Pointer<Void>, Int32);
typedef _ReadyD = int Function(Pointer<Void>, int);
typedef _WaitC = Int32 Function(
    Pointer<Void>, Int32, Double, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _WaitD = int Function(
    Pointer<Void>, int, double, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _CountersC = Int32 Function(Pointer<Void>, Pointer<TshCounters>);
typedef _CountersD = int Function(Pointer<Void>, Pointer<TshCounters>);
typedef _ScanF16StatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _ScanF16StatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _ProbeScanF16C = Int32 Function(Pointer<Void>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _ProbeScanF16D = int Function(Pointer<Void>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _ScanI8StatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _ScanI8StatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchAfterC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Double, Pointer<Uint8>,
    Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchAfterD = int Function(Pointer<Void>, Pointer<Float>, int, int, double, Pointer<Uint8>,
    Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SubmitAfterC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Pointer<Uint8>, Pointer<Void>,
    Double, Int64, Pointer<Int32>);
typedef _SubmitAfterD = int Function(Pointer<Void>, Pointer<Float>, int, Pointer<Uint8>, Pointer<Void>,
    double, int, Pointer<Int32>);
typedef _SearchAfterStatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchAfterStatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchCountC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Double>, Pointer<Int64>, Pointer<Int64>);
typedef _SearchCountD = int Function(Pointer<Void>, Pointer<Float>, int, double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Double>, Pointer<Int64>, Pointer<Int64>);
typedef _SearchCountStatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchCountStatsD = int Function(Pointer<Void>, Pointer<Int64>);
// (the last argument is the address of the handle to fill: the header declares it void *)
typedef _GroupsCreateC = Int32 Function(Pointer<Void>, Pointer<Int32>, Int64, Int32, Pointer<Void>);
typedef _GroupsCreateD = int Function(Pointer<Void>, Pointer<Int32>, int, int, Pointer<Void>);
typedef _GroupsSetC = Int32 Function(Pointer<Void>, Int64, Int64, Pointer<Int32>);
typedef _GroupsSetD = int Function(Pointer<Void>, int, int, Pointer<Int32>);
typedef _GroupsDestroyC = Int32 Function(Pointer<Void>);
typedef _GroupsDestroyD = int Function(Pointer<Void>);
typedef _SearchGroupedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchGroupedD = int Function(Pointer<Void>, Pointer<Float>, int, int, double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchGroupedStatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchGroupedStatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchGroupedAfterC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchGroupedAfterD = int Function(Pointer<Void>, Pointer<Float>, int, int, double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchGroupedCountC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>);
typedef _SearchGroupedCountD = int Function(Pointer<Void>, Pointer<Float>, int, double, Pointer<Uint8>, Pointer<Void>,
    Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>);
typedef _SearchGroupedAfterStatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchGroupedAfterStatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchGroupedRowsC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Int32, Double, Pointer<Uint8>,
    Pointer<Void>, Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchGroupedRowsD = int Function(Pointer<Void>, Pointer<Float>, int, int, int, double, Pointer<Uint8>,
    Pointer<Void>, Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchGroupedRowsStatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _SearchGroupedRowsStatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _ProbeScanI8C = Int32 Function(Pointer<Void>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _ProbeScanI8D = int Function(Pointer<Void>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _ScanI4StatsC = Int32 Function(Pointer<Void>, Pointer<Int64>);
typedef _ScanI4StatsD = int Function(Pointer<Void>, Pointer<Int64>);
typedef _ProbeScanI4C = Int32 Function(Pointer<Void>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _ProbeScanI4D = int Function(Pointer<Void>, Pointer<Float>, Pointer<Float>, Pointer<Float>);
typedef _SetOptionC = Int32 Function(Pointer<Void>, Int32, Int64);
typedef _SetOptionD = int Function(Pointer<Void>, int, int);
typedef _BlockBytesC = Int64 Function(Int32);
typedef _BlockBytesD = int Function(int);
typedef _BlockEntriesC = Int32 Function(Int32);
typedef _BlockEntriesD = int Function(int);
typedef _SearchShardC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Uint8>,
    Int32, Pointer<Void>, Pointer<Void>);
typedef _SearchShardD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Uint8>,
    int, Pointer<Void>, Pointer<Void>);
typedef _ShardBeginC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Uint8>,
    Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _ShardBeginD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Uint8>,
    int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _ShardProgressC = Int32 Function(Pointer<Void>, Int32, Pointer<Int32>);
typedef _ShardProgressD = int Function(Pointer<Void>, int, Pointer<Int32>);
typedef _ShardEndC = Int32 Function(Pointer<Void>);
typedef _ShardEndD = int Function(Pointer<Void>);
typedef _MergeC = Int32 Function(Int32, Int32, Pointer<Float>, Int32, Int32, Double, Pointer<Void>,
    Int32, Int32, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _MergeD = int Function(int, int, Pointer<Float>, int, int, double, Pointer<Void>,
    int, int, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _CommIdC = Int32 Function(Pointer<Void>);
typedef _CommIdD = int Function(Pointer<Void>);
typedef _CommCreateC = Int32 Function(Pointer<Void>, Int32, Int32, Int32, Pointer<Pointer<Void>>);
typedef _CommCreateD = int Function(Pointer<Void>, int, int, int, Pointer<Pointer<Void>>);
/// `tsh_allgather_fn`: int32 (*)(void *user, const void *send, void *recv, int64 bytes)
typedef TshAllgatherNative = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Void>, Int64);
typedef _CommCreateHostC = Int32 Function(Int32, Int32, Int32,
    Pointer<NativeFunction<TshAllgatherNative>>, Pointer<Void>, Pointer<Pointer<Void>>);
typedef _CommCreateHostD = int Function(int, int, int,
    Pointer<NativeFunction<TshAllgatherNative>>, Pointer<Void>, Pointer<Pointer<Void>>);
typedef _CommDestroyC = Int32 Function(Pointer<Void>);
typedef _CommDestroyD = int Function(Pointer<Void>);
typedef _CommWorldC = Int32 Function(Pointer<Void>);
typedef _CommWorldD = int Function(Pointer<Void>);
typedef _CommSetGroupC = Int32 Function(Pointer<Void>, Int32);
typedef _CommSetGroupD = int Function(Pointer<Void>, int);
typedef _CommTimelineC = Int32 Function(Pointer<Void>, Pointer<TshCommTimeline>, Int32);
typedef _CommTimelineD = int Function(Pointer<Void>, Pointer<TshCommTimeline>, int);
typedef _SearchShardedC = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, Int32, Int32,
    Double, Pointer<Uint8>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchShardedD = int Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, int, int,
    double, Pointer<Uint8>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchShardAfterC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Uint8>,
    Pointer<Double>, Pointer<Int64>, Int32, Pointer<Void>, Pointer<Void>);
typedef _SearchShardAfterD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Uint8>,
    Pointer<Double>, Pointer<Int64>, int, Pointer<Void>, Pointer<Void>);
typedef _ShardBeginAfterC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Uint8>,
    Pointer<Double>, Pointer<Int64>, Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _ShardBeginAfterD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Uint8>,
    Pointer<Double>, Pointer<Int64>, int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _MergeAfterC = Int32 Function(Int32, Int32, Pointer<Float>, Int32, Int32, Double, Pointer<Double>,
    Pointer<Int64>, Pointer<Void>, Int32, Int32, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _MergeAfterD = int Function(int, int, Pointer<Float>, int, int, double, Pointer<Double>,
    Pointer<Int64>, Pointer<Void>, int, int, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchShardedAfterC = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, Int32, Int32,
    Double, Pointer<Uint8>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchShardedAfterD = int Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, int, int,
    double, Pointer<Uint8>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchShardGroupedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Uint8>,
    Pointer<Void>, Pointer<Void>, Int32, Pointer<Void>, Pointer<Void>);
typedef _SearchShardGroupedD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Uint8>,
    Pointer<Void>, Pointer<Void>, int, Pointer<Void>, Pointer<Void>);
typedef _ShardBeginGroupedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Uint8>,
    Pointer<Void>, Pointer<Void>, Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _ShardBeginGroupedD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Uint8>,
    Pointer<Void>, Pointer<Void>, int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _MergeGroupedC = Int32 Function(Int32, Int32, Pointer<Float>, Int32, Int32, Double, Pointer<Int32>,
    Int64, Pointer<Void>, Int32, Int32, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>, Pointer<Int32>);
typedef _MergeGroupedD = int Function(int, int, Pointer<Float>, int, int, double, Pointer<Int32>,
    int, Pointer<Void>, int, int, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchShardedGroupedC = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, Int32, Int32,
    Double, Pointer<Uint8>, Pointer<Void>, Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchShardedGroupedD = int Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, int, int,
    double, Pointer<Uint8>, Pointer<Void>, Pointer<Void>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>, Pointer<Int32>);
typedef _SearchShardMaskedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Void>,
    Pointer<Double>, Pointer<Int64>, Int32, Pointer<Void>, Pointer<Void>);
typedef _SearchShardMaskedD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Void>,
    Pointer<Double>, Pointer<Int64>, int, Pointer<Void>, Pointer<Void>);
typedef _ShardBeginMaskedC = Int32 Function(Pointer<Void>, Pointer<Float>, Int32, Int32, Pointer<Void>,
    Pointer<Double>, Pointer<Int64>, Int32, Pointer<Void>, Int32, Pointer<Pointer<Void>>);
typedef _ShardBeginMaskedD = int Function(Pointer<Void>, Pointer<Float>, int, int, Pointer<Void>,
    Pointer<Double>, Pointer<Int64>, int, Pointer<Void>, int, Pointer<Pointer<Void>>);
typedef _SearchShardedMaskedC = Int32 Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, Int32, Int32,
    Double, Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);
typedef _SearchShardedMaskedD = int Function(Pointer<Void>, Pointer<Void>, Pointer<Float>, int, int,
    double, Pointer<Void>, Pointer<Double>, Pointer<Int64>, Pointer<Int64>, Pointer<Double>, Pointer<Int32>);

/// `tsh_counters` (include/tostore_hip.h).  Field order and widths are checked against the header by
/// tests/test_dart_bridge.py.
final class TshCounters extends Struct {
  @Int64()
  external int rows;
  @Int64()
  external int deletedRows;
  @Int64()
  external int searches;
  @Int64()
  external int scanLaunches;
  @Int64()
  external int batchLaunches;
  @Int64()
  external int fallbackSearches;
  @Int64()
  external int candidatesTotal;
  @Int64()
  external int bytesResident;
  @Int32()
  external int safeMode;
  @Int32()
  external int deviceId;
  @Double()
  external double scanUsSum;
  @Int64()
  external int scanUsSamples;
  @Int32()
  external int batchKernelLast;
  @Int32()
  external int quarantinedRows;
  @Int64()
  external int exactScans;
  @Int64()
  external int batchPlaneFallbacks;
  @Int64()
  external int batchScanFallbacks;
  @Int64()
  external int listScans;
  @Int64()
  external int exactRedone;
}

/// `tsh_comm_timeline` (include/tostore_hip.h): where this rank's tsh_search_sharded time went.  Field order and
/// widths are checked against the header by tests/test_dart_bridge.py.
final class TshCommTimeline extends Struct {
  @Int64()
  external int calls;
  @Int64()
  external int queries;
  @Int64()
  external int groups;
  @Int64()
  external int retries;
  @Int32()
  external int world;
  @Int32()
  external int rank;
  @Int32()
  external int transport;
  @Int32()
  external int reserved;
  @Double()
  external double callUs;
  @Double()
  external double reserveUs;
  @Double()
  external double waitScanUs;
  @Double()
  external double scanUs;
  @Double()
  external double exchangeWaitUs;
  @Double()
  external double gatherUs;
  @Double()
  external double sliceD2hUs;
  @Double()
  external double mergeUs;
  @Double()
  external double resultGatherUs;
  @Double()
  external double copyOutUs;
  @Double()
  external double retryScanUs;
  @Double()
  external double preEnqueueUs;
}

/// `tsh_ngh_info` (include/tostore_hip.h): what tsh_index_open_ngh found.  Field order and
/// widths are checked against the header by tests/test_dart_bridge.py.
final class TshNghInfo extends Struct {
  @Int32()
  external int dimensions;
  @Int32()
  external int metric;
  @Int32()
  external int precision;
  @Int32()
  external int pageSize;
  @Int32()
  external int maxDegree;
  @Int32()
  external int reserved;
  @Int64()
  external int nextNodeId;
  @Int64()
  external int totalVectors;
  @Int64()
  external int deletedCount;
  @Int64()
  external int maxPartitionFileSize;
  @Int64()
  external int rowsLoaded;
  @Int64()
  external int tombstones;
  @Int64()
  external int filesRead;
  @Int64()
  external int pagesAbsent;
  @Int64()
  external int filesAbsent;
  @Int64()
  external int rowBase;
  @Int64()
  external int rowEnd;
}

/// `tsh_where_term` (include/tostore_hip.h): one term of a tsh_mask_create_where call, 56 bytes.  Field order and
/// widths are checked against the header by tests/test_abi_mask_where_terms.py.
final class TshWhereTerm extends Struct {
  external Pointer<Void> attr;
  @Int64()
  external int lo;
  @Int64()
  external int hi;
  external Pointer<Int64> set;
  @Int64()
  external int nSet;
  @Int32()
  external int kind;
  @Int32()
  external int negate;
  @Int32()
  external int clause;
  @Int32()
  external int reserved;
}

/// A term of [HipRowMask.whereClauses]: a range term keeps the node ids whose attribute is not NULL and for which
/// (lo <= value <= hi) != negate; a set term ([HipWhereTerm.inSet]) those for which (value in values) != negate.
final class HipWhereTerm {
  final HipRowAttr attr;
  final int lo, hi;
  final Int64List? values;
  final bool negate;
  const HipWhereTerm.range(this.attr, this.lo, this.hi, {this.negate = false}) : values = null;
  HipWhereTerm.inSet(this.attr, Int64List this.values, {this.negate = false})
      : lo = 0,
        hi = 0;
}

/// One device-resident copy of an NGH index's raw-vector column.
///
/// Lifetime: created lazily on the first vectorSearch / writeChanges of
/// (tableName, indexName); dropped from clearCacheForTable / clearCacheForIndex /
/// dispose (vector_index_manager.dart:1192-1216) and after reorderByLocality
/// (:932-1159), which renumbers node ids.
final class HipVectorBackend {
  static DynamicLibrary? _lib;
  static bool _probed = false;

  static late final _AbiVersionD _abiVersion;
  static late final _DeviceCountD _deviceCount;
  static late final _LastErrorD _lastError;
  static late final _CreateD _create;
  static late final _DestroyD _destroy;
  static late final _AppendD _append;
  static late final _SetDeletedD _setDeleted;
  static late final _LoadRawvecD _loadRawvec;
  static late final _SizeD _size;
  static late final _SearchD _search;
  static late final _OpenNghD _openNgh;
  static late final _PqEncodeD _pqEncode;
  static late final _PqTrainD _pqTrain;
  static late final _CreateShardD _createShard;
  static late final _DimD _dim;
  static late final _MetricD _metric;
  static late final _MaxInflightD _maxInflight;
  static late final _SubmitD _submit;
  static late final _ReadyD _ready;
  static late final _WaitD _wait;
  static late final _CountersD _counters;
  static late final _SetOptionD _setOption;
  static late final _ScanF16StatsD _scanF16Stats;
  static late final _ProbeScanF16D _probeScanF16;
  static late final _ScanI8StatsD _scanI8Stats;
  static late final _SearchAfterD _searchAfter;
  static late final _SubmitAfterD _submitAfter;
  static late final _SearchAfterStatsD _searchAfterStats;
  static late final _SearchCountD _searchCount;
  static late final _SearchCountStatsD _searchCountStats;
  static late final _GroupsCreateD _groupsCreate;
  static late final _GroupsSetD _groupsSet;
  static late final _GroupsDestroyD _groupsDestroy;
  static late final _SearchGroupedD _searchGrouped;
  static late final _SearchGroupedStatsD _searchGroupedStats;
  static late final _SearchGroupedAfterD _searchGroupedAfter;
  static late final _SearchGroupedCountD _searchGroupedCount;
  static late final _SearchGroupedAfterStatsD _searchGroupedAfterStats;
  static late final _SearchGroupedRowsD _searchGroupedRows;
  static late final _SearchGroupedRowsStatsD _searchGroupedRowsStats;
  static late final _ProbeScanI8D _probeScanI8;
  static late final _ScanI4StatsD _scanI4Stats;
  static late final _ProbeScanI4D _probeScanI4;
  static late final _BlockBytesD _blockBytes;
  static late final _BlockEntriesD _blockEntries;
  static late final _SearchShardD _searchShard;
  static late final _ShardBeginD _shardBegin;
  static late final _ShardProgressD _shardProgress;
  static late final _ShardEndD _shardEnd;
  static late final _MergeD _merge;
  static late final _CommIdD _commId;
  static late final _CommCreateD _commCreate;
  static late final _CommCreateHostD _commCreateHost;
  static late final _CommDestroyD _commDestroy;
  static late final _CommWorldD _commWorld;
  static late final _CommSetGroupD _commSetGroup;
  static late final _SearchShardedD _searchSharded;
  static late final _SearchShardAfterD _searchShardAfter;
  static late final _ShardBeginAfterD _shardBeginAfter;
  static late final _MergeAfterD _mergeAfter;
  static late final _SearchShardedAfterD _searchShardedAfter;
  static late final _SearchShardGroupedD _searchShardGrouped;
  static late final _ShardBeginGroupedD _shardBeginGrouped;
  static late final _MergeGroupedD _mergeGrouped;
  static late final _SearchShardedGroupedD _searchShardedGrouped;
  static late final _SearchShardMaskedD _searchShardMasked;
  static late final _ShardBeginMaskedD _shardBeginMasked;
  static late final _SearchShardedMaskedD _searchShardedMasked;
  static late final _CommTimelineD _commTimeline;
  static late final _OpenNghShardD _openNghShard;
  static late final _MaskCreateD _maskCreate;
  static late final _MaskDestroyD _maskDestroy;
  static late final _MaskKeptD _maskKept;
  static late final _AttrCreateD _attrCreate;
  static late final _AttrSetD _attrSet;
  static late final _AttrDestroyD _attrDestroy;
  static late final _MaskCreateRangeD _maskCreateRange;
  static late final _MaskReadD _maskRead;
  static late final _MaskCreateWhereD _maskCreateWhere;
  static late final _TagsCreateD _tagsCreate;
  static late final _TagsSetD _tagsSet;
  static late final _TagsDestroyD _tagsDestroy;
  static late final _MaskCreateTagsD _maskCreateTags;
  static late final _AttrFacetsD _attrFacets;
  static late final _TagsFacetsD _tagsFacets;
  static late final _SearchMaskedD _searchMasked;
  static late final _SubmitMaskedD _submitMasked;

  /// include/tostore_hip.h TSH_ABI_VERSION this file was written against.
  static const int abiVersion = 5;

  /// True when libtostore_hip.so is loadable, ABI-compatible and sees a GPU.
  static bool get available {
    if (_probed) return _lib != null;
    _probed = true;
    try {
      final lib = DynamicLibrary.open('libtostore_hip.so');
      _abiVersion = lib.lookupFunction<_AbiVersionC, _AbiVersionD>('tsh_abi_version');
      _deviceCount = lib.lookupFunction<_DeviceCountC, _DeviceCountD>('tsh_device_count');
      _lastError = lib.lookupFunction<_LastErrorC, _LastErrorD>('tsh_last_error');
      _create = lib.lookupFunction<_CreateC, _CreateD>('tsh_index_create');
      _destroy = lib.lookupFunction<_DestroyC, _DestroyD>('tsh_index_destroy');
      _append = lib.lookupFunction<_AppendC, _AppendD>('tsh_index_append');
      _setDeleted = lib.lookupFunction<_SetDeletedC, _SetDeletedD>('tsh_index_set_deleted');
      _loadRawvec =
          lib.lookupFunction<_LoadRawvecC, _LoadRawvecD>('tsh_index_load_rawvec_file');
      _size = lib.lookupFunction<_SizeC, _SizeD>('tsh_index_size');
      _search = lib.lookupFunction<_SearchC, _SearchD>('tsh_search');
      _openNgh = lib.lookupFunction<_OpenNghC, _OpenNghD>('tsh_index_open_ngh');
      _pqEncode = lib.lookupFunction<_PqEncodeC, _PqEncodeD>('tsh_index_pq_encode');
      _pqTrain = lib.lookupFunction<_PqTrainC, _PqTrainD>('tsh_pq_train');
      _createShard = lib.lookupFunction<_CreateShardC, _CreateShardD>('tsh_index_create_shard');
      _dim = lib.lookupFunction<_DimC, _DimD>('tsh_index_dim');
      _metric = lib.lookupFunction<_MetricC, _MetricD>('tsh_index_metric');
      _maxInflight = lib.lookupFunction<_MaxInflightC, _MaxInflightD>('tsh_max_inflight');
      _submit = lib.lookupFunction<_SubmitC, _SubmitD>('tsh_search_submit');
      _ready = lib.lookupFunction<_ReadyC, _ReadyD>('tsh_search_ready');
      _wait = lib.lookupFunction<_WaitC, _WaitD>('tsh_search_wait');
      _counters = lib.lookupFunction<_CountersC, _CountersD>('tsh_get_counters');
      _setOption = lib.lookupFunction<_SetOptionC, _SetOptionD>('tsh_index_set_option');
      _scanF16Stats = lib.lookupFunction<_ScanF16StatsC, _ScanF16StatsD>('tsh_scan_f16_stats');
      _probeScanF16 = lib.lookupFunction<_ProbeScanF16C, _ProbeScanF16D>('tsh_probe_scan_f16_keys');
      _scanI8Stats = lib.lookupFunction<_ScanI8StatsC, _ScanI8StatsD>('tsh_scan_i8_stats');
      _searchAfter = lib.lookupFunction<_SearchAfterC, _SearchAfterD>('tsh_search_after');
      _submitAfter = lib.lookupFunction<_SubmitAfterC, _SubmitAfterD>('tsh_search_submit_after');
      _searchAfterStats =
          lib.lookupFunction<_SearchAfterStatsC, _SearchAfterStatsD>('tsh_search_after_stats');
      _searchCount = lib.lookupFunction<_SearchCountC, _SearchCountD>('tsh_search_count');
      _searchCountStats =
          lib.lookupFunction<_SearchCountStatsC, _SearchCountStatsD>('tsh_search_count_stats');
      _groupsCreate = lib.lookupFunction<_GroupsCreateC, _GroupsCreateD>('tsh_groups_create');
      _groupsSet = lib.lookupFunction<_GroupsSetC, _GroupsSetD>('tsh_groups_set');
      _groupsDestroy = lib.lookupFunction<_GroupsDestroyC, _GroupsDestroyD>('tsh_groups_destroy');
      _searchGrouped = lib.lookupFunction<_SearchGroupedC, _SearchGroupedD>('tsh_search_grouped');
      _searchGroupedStats =
          lib.lookupFunction<_SearchGroupedStatsC, _SearchGroupedStatsD>('tsh_search_grouped_stats');
      _searchGroupedAfter =
          lib.lookupFunction<_SearchGroupedAfterC, _SearchGroupedAfterD>('tsh_search_grouped_after');
      _searchGroupedCount =
          lib.lookupFunction<_SearchGroupedCountC, _SearchGroupedCountD>('tsh_search_grouped_count');
      _searchGroupedAfterStats =
          lib.lookupFunction<_SearchGroupedAfterStatsC, _SearchGroupedAfterStatsD>('tsh_search_grouped_after_stats');
      _searchGroupedRows =
          lib.lookupFunction<_SearchGroupedRowsC, _SearchGroupedRowsD>('tsh_search_grouped_rows');
      _searchGroupedRowsStats =
          lib.lookupFunction<_SearchGroupedRowsStatsC, _SearchGroupedRowsStatsD>('tsh_search_grouped_rows_stats');
      _probeScanI8 = lib.lookupFunction<_ProbeScanI8C, _ProbeScanI8D>('tsh_probe_scan_i8_keys');
      _scanI4Stats = lib.lookupFunction<_ScanI4StatsC, _ScanI4StatsD>('tsh_scan_i4_stats');
      _probeScanI4 = lib.lookupFunction<_ProbeScanI4C, _ProbeScanI4D>('tsh_probe_scan_i4_keys');
      _blockBytes = lib.lookupFunction<_BlockBytesC, _BlockBytesD>('tsh_candidate_block_bytes');
      _blockEntries = lib.lookupFunction<_BlockEntriesC, _BlockEntriesD>('tsh_default_block_entries');
      _searchShard = lib.lookupFunction<_SearchShardC, _SearchShardD>('tsh_search_shard');
      _shardBegin = lib.lookupFunction<_ShardBeginC, _ShardBeginD>('tsh_search_shard_begin');
      _shardProgress =
          lib.lookupFunction<_ShardProgressC, _ShardProgressD>('tsh_search_shard_progress');
      _shardEnd = lib.lookupFunction<_ShardEndC, _ShardEndD>('tsh_search_shard_end');
      _merge = lib.lookupFunction<_MergeC, _MergeD>('tsh_merge_candidates');
      _commId = lib.lookupFunction<_CommIdC, _CommIdD>('tsh_comm_unique_id');
      _commCreate = lib.lookupFunction<_CommCreateC, _CommCreateD>('tsh_comm_create');
      _commCreateHost =
          lib.lookupFunction<_CommCreateHostC, _CommCreateHostD>('tsh_comm_create_host');
      _commDestroy = lib.lookupFunction<_CommDestroyC, _CommDestroyD>('tsh_comm_destroy');
      _commWorld = lib.lookupFunction<_CommWorldC, _CommWorldD>('tsh_comm_world');
      _commSetGroup = lib.lookupFunction<_CommSetGroupC, _CommSetGroupD>('tsh_comm_set_group');
      _searchSharded =
          lib.lookupFunction<_SearchShardedC, _SearchShardedD>('tsh_search_sharded');
      _searchShardAfter =
          lib.lookupFunction<_SearchShardAfterC, _SearchShardAfterD>('tsh_search_shard_after');
      _shardBeginAfter =
          lib.lookupFunction<_ShardBeginAfterC, _ShardBeginAfterD>('tsh_search_shard_begin_after');
      _mergeAfter = lib.lookupFunction<_MergeAfterC, _MergeAfterD>('tsh_merge_candidates_after');
      _searchShardedAfter =
          lib.lookupFunction<_SearchShardedAfterC, _SearchShardedAfterD>('tsh_search_sharded_after');
      _searchShardGrouped =
          lib.lookupFunction<_SearchShardGroupedC, _SearchShardGroupedD>('tsh_search_shard_grouped');
      _shardBeginGrouped =
          lib.lookupFunction<_ShardBeginGroupedC, _ShardBeginGroupedD>('tsh_search_shard_begin_grouped');
      _mergeGrouped = lib.lookupFunction<_MergeGroupedC, _MergeGroupedD>('tsh_merge_candidates_grouped');
      _searchShardedGrouped =
          lib.lookupFunction<_SearchShardedGroupedC, _SearchShardedGroupedD>('tsh_search_sharded_grouped');
      _searchShardMasked =
          lib.lookupFunction<_SearchShardMaskedC, _SearchShardMaskedD>('tsh_search_shard_masked');
      _shardBeginMasked =
          lib.lookupFunction<_ShardBeginMaskedC, _ShardBeginMaskedD>('tsh_search_shard_begin_masked');
      _searchShardedMasked =
          lib.lookupFunction<_SearchShardedMaskedC, _SearchShardedMaskedD>('tsh_search_sharded_masked');
      _commTimeline =
          lib.lookupFunction<_CommTimelineC, _CommTimelineD>('tsh_comm_get_timeline');
      _openNghShard =
          lib.lookupFunction<_OpenNghShardC, _OpenNghShardD>('tsh_index_open_ngh_shard');
      _maskCreate = lib.lookupFunction<_MaskCreateC, _MaskCreateD>('tsh_mask_create');
      _maskDestroy = lib.lookupFunction<_MaskDestroyC, _MaskDestroyD>('tsh_mask_destroy');
      _maskKept = lib.lookupFunction<_MaskKeptC, _MaskKeptD>('tsh_mask_kept');
      _attrCreate = lib.lookupFunction<_AttrCreateC, _AttrCreateD>('tsh_attr_create');
      _attrSet = lib.lookupFunction<_AttrSetC, _AttrSetD>('tsh_attr_set');
      _attrDestroy = lib.lookupFunction<_AttrDestroyC, _AttrDestroyD>('tsh_attr_destroy');
      _maskCreateRange = lib.lookupFunction<_MaskCreateRangeC, _MaskCreateRangeD>('tsh_mask_create_range');
      _maskRead = lib.lookupFunction<_MaskReadC, _MaskReadD>('tsh_mask_read');
      _maskCreateWhere = lib.lookupFunction<_MaskCreateWhereC, _MaskCreateWhereD>('tsh_mask_create_where');
      _tagsCreate = lib.lookupFunction<_TagsCreateC, _TagsCreateD>('tsh_tags_create');
      _tagsSet = lib.lookupFunction<_TagsSetC, _TagsSetD>('tsh_tags_set');
      _tagsDestroy = lib.lookupFunction<_TagsDestroyC, _TagsDestroyD>('tsh_tags_destroy');
      _maskCreateTags = lib.lookupFunction<_MaskCreateTagsC, _MaskCreateTagsD>('tsh_mask_create_tags');
      _attrFacets = lib.lookupFunction<_AttrFacetsC, _AttrFacetsD>('tsh_attr_facets');
      _tagsFacets = lib.lookupFunction<_TagsFacetsC, _TagsFacetsD>('tsh_tags_facets');
      _searchMasked = lib.lookupFunction<_SearchMaskedC, _SearchMaskedD>('tsh_search_masked');
      _submitMasked =
          lib.lookupFunction<_SubmitMaskedC, _SubmitMaskedD>('tsh_search_submit_masked');
      // the structs of this file are the version-5 layouts: any other library is not used
      if (_abiVersion() != abiVersion || _deviceCount() < 1) return false;
      _lib = lib;
      return true;
    } catch (_) {
      return false; // same catch-and-fall-back style as SystemFFIHelper
    }
  }

  static String _errorText() {
    final buf = calloc<Uint8>(512);
    try {
      _lastError(buf.cast<Utf8>(), 512);
      return buf.cast<Utf8>().toDartString();
    } finally {
      calloc.free(buf);
    }
  }

  Pointer<Void> _handle;
  final int dimensions;
  final VectorDistanceMetric metric;

  HipVectorBackend._(this._handle, this.dimensions, this.metric);

  /// metric index = enum order of VectorDistanceMetric (table_schema.dart:2511-2531).
  static HipVectorBackend? tryCreate(NghIndexMeta meta, {int devices = 1}) {
    if (!available) return null;
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _create(meta.dimensions, meta.distanceMetric.index,
          meta.nextNodeId > 0 ? meta.nextNodeId : 0, devices, out);
      if (rc != 0) {
        Logger.warn('tsh_index_create failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      return HipVectorBackend._(out.value, meta.dimensions, meta.distanceMetric);
    } finally {
      calloc.free(out);
    }
  }

  /// Cold start straight from `<index>/ngh` (path_manager.dart:275-278): the library reads
  /// meta.json, every rawvec partition and the graph slots' deleted flags itself.
  static HipVectorBackend? tryOpen(String nghDir, NghIndexMeta meta, int maxEntriesPerDir,
      {int devices = 1}) {
    if (!available) return null;
    final out = calloc<Pointer<Void>>();
    final info = calloc<TshNghInfo>();
    final p = nghDir.toNativeUtf8();
    try {
      final rc = _openNgh(p, maxEntriesPerDir, devices, out, info);
      if (rc != 0) {
        Logger.warn('tsh_index_open_ngh failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      // Raw-vector pages that are not on disk load as ABSENT rows: the exhaustive path would
      // silently never return those nodes, so an index with holes stays on the Dart path.
      if (info.ref.pagesAbsent != 0 || info.ref.rowsLoaded != meta.nextNodeId) {
        Logger.warn(
            'device index of $nghDir not used: ${info.ref.pagesAbsent} raw-vector pages absent, '
            '${info.ref.rowsLoaded} of ${meta.nextNodeId} rows loaded',
            label: 'HipVectorBackend');
        _destroy(out.value);
        return null;
      }
      return HipVectorBackend._(out.value, meta.dimensions, meta.distanceMetric);
    } finally {
      calloc.free(p);
      calloc.free(info);
      calloc.free(out);
    }
  }

  /// Cold start of ONE rank's row range of `<index>/ngh` (one Dart process per GPU, [HipShardComm]): node ids
  /// [rank * ceil(nextNodeId / world), ...) as a shard handle with global ids -- the library opens only the
  /// partition files and reads only the pages that hold the range (model/ngh_index_meta.dart:480-490,
  /// core/path_manager.dart:275-324).  Null when the range has holes on disk, like [tryOpen].
  static HipVectorBackend? tryOpenShard(String nghDir, NghIndexMeta meta, int maxEntriesPerDir,
      int device, int world, int rank) {
    if (!available) return null;
    final out = calloc<Pointer<Void>>();
    final info = calloc<TshNghInfo>();
    final p = nghDir.toNativeUtf8();
    try {
      final rc = _openNghShard(p, maxEntriesPerDir, device, world, rank, out, info);
      if (rc != 0) {
        Logger.warn('tsh_index_open_ngh_shard failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      final want = info.ref.rowEnd - info.ref.rowBase;
      if (info.ref.pagesAbsent != 0 || info.ref.rowsLoaded != want) {
        Logger.warn(
            'device shard $rank/$world of $nghDir not used: ${info.ref.pagesAbsent} raw-vector pages '
            'absent, ${info.ref.rowsLoaded} of $want rows loaded',
            label: 'HipVectorBackend');
        _destroy(out.value);
        return null;
      }
      return HipVectorBackend._(out.value, meta.dimensions, meta.distanceMetric);
    } finally {
      calloc.free(p);
      calloc.free(info);
      calloc.free(out);
    }
  }

  /// A WHERE row set that lives on the device across queries (tsh_mask_create): bit i of `bits` (LSB first)
  /// keeps node id i.  The bitmap crosses the FFI boundary ONCE; searches that pass the handle
  /// ([search] / [searchAsync] `mask:`) copy nothing and do no host work on it -- the `rowMask:` form
  /// callocs, copies and has the library slice, count and list the bitmap on every call.  Dispose the mask
  /// before this backend.
  HipRowMask? createMask(Uint8List bits) {
    final buf = calloc<Uint8>(bits.isEmpty ? 1 : bits.length);
    final out = calloc<Pointer<Void>>();
    try {
      buf.asTypedList(bits.length).setAll(0, bits);
      final rc = _maskCreate(_handle, buf, bits.length, out);
      if (rc != 0) {
        Logger.warn('tsh_mask_create failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipRowMask._(out.value);
    } finally {
      calloc.free(buf);
      calloc.free(out);
    }
  }

  /// One scalar attribute of every node id, kept on the device (tsh_attr_create): entry i of `values` belongs to node
  /// id i, [HipRowAttr.nullValue] says the row has none, rows beyond the list read as NULL.  The column crosses the FFI
  /// boundary once; [HipRowAttr.set] extends it as rows are appended.  Doubles and DateTimes go in by
  /// [HipRowAttr.doubleKey].  Dispose it before this backend.
  HipRowAttr? createAttr(Int64List values) {
    final buf = calloc<Int64>(values.isEmpty ? 1 : values.length);
    final out = calloc<Pointer<Void>>();
    try {
      buf.asTypedList(values.length).setAll(0, values);
      final rc = _attrCreate(_handle, buf, values.length, out.cast<Void>());
      if (rc != 0) {
        Logger.warn('tsh_attr_create failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipRowAttr._(out.value);
    } finally {
      calloc.free(buf);
      calloc.free(out);
    }
  }

  /// A mask made ON the device from one range term (tsh_mask_create_range): keeps the node ids whose attribute is not
  /// NULL and for which (lo <= value <= hi) != negate, and-ed (or, with `or: true`, or-ed) with `withMask` when one is
  /// given.  lo > hi is the empty range.  `tenant IN (3, 7) AND ts BETWEEN a AND b AND NOT flag` is a chain of calls, each
  /// returning a new mask; dispose the intermediates.  The mask is a snapshot: later [HipRowAttr.set] calls and appends
  /// do not change it.  Null on any native failure; a disposed [HipRowAttr] or `withMask` is refused (null, with a
  /// warning), never sent as NULL.
  HipRowMask? createMaskWhere(HipRowAttr attr, int lo, int hi, {bool negate = false, HipRowMask? withMask, bool or = false}) {
    if (attr._attr == nullptr) {
      Logger.warn('createMaskWhere with a disposed HipRowAttr', label: 'HipVectorBackend');
      return null;
    }
    if (withMask != null && withMask._mask == nullptr) {
      Logger.warn('createMaskWhere with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _maskCreateRange(_handle, attr._attr, lo, hi, negate ? 1 : 0, withMask?._mask ?? nullptr, or ? 1 : 0, out);
      if (rc != 0) {
        Logger.warn('tsh_mask_create_range failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipRowMask._(out.value);
    } finally {
      calloc.free(out);
    }
  }

  /// A mask made ON the device from a whole WHERE in one launch (tsh_mask_create_where): `clauses` is a list of clauses,
  /// each a list of [HipWhereTerm]s; a clause is the OR of its terms and the result the AND of the clauses, and-ed (or,
  /// with `or: true`, or-ed) with `withMask` when one is given.  At most [whereMaxTerms] terms over [whereMaxColumns]
  /// attributes and [whereMaxSetValues] set values; more is chained through `withMask`.  A snapshot, as
  /// [createMaskWhere]'s.  Null on any native failure; a disposed [HipRowAttr] or `withMask` is refused (null, with a
  /// warning), never sent as NULL.
  HipRowMask? createMaskWhereClauses(List<List<HipWhereTerm>> clauses, {HipRowMask? withMask, bool or = false}) {
    final flat = <HipWhereTerm>[];
    final clauseOf = <int>[];
    for (var c = 0; c < clauses.length; c++) {
      for (final t in clauses[c]) {
        if (t.attr._attr == nullptr) {
          Logger.warn('createMaskWhereClauses with a disposed HipRowAttr', label: 'HipVectorBackend');
          return null;
        }
        flat.add(t);
        clauseOf.add(c);
      }
    }
    if (withMask != null && withMask._mask == nullptr) {
      Logger.warn('createMaskWhereClauses with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    final terms = calloc<TshWhereTerm>(flat.isEmpty ? 1 : flat.length);
    final sets = <Pointer<Int64>>[];
    final out = calloc<Pointer<Void>>();
    try {
      for (var i = 0; i < flat.length; i++) {
        final t = flat[i];
        final rec = terms[i];
        rec.attr = t.attr._attr;
        rec.lo = t.lo;
        rec.hi = t.hi;
        rec.negate = t.negate ? 1 : 0;
        rec.clause = clauseOf[i];
        rec.reserved = 0;
        final v = t.values;
        if (v == null) {
          rec.kind = termRange;
          rec.set = nullptr;
          rec.nSet = 0;
        } else {
          final buf = calloc<Int64>(v.isEmpty ? 1 : v.length);
          buf.asTypedList(v.length).setAll(0, v);
          sets.add(buf);
          rec.kind = termIn;
          rec.set = buf;
          rec.nSet = v.length;
        }
      }
      final rc = _maskCreateWhere(_handle, terms.cast<Void>(), flat.length, withMask?._mask ?? nullptr, or ? 1 : 0, out);
      if (rc != 0) {
        Logger.warn('tsh_mask_create_where failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipRowMask._(out.value);
    } finally {
      for (final s in sets) {
        calloc.free(s);
      }
      calloc.free(terms);
      calloc.free(out);
    }
  }

  /// One array-valued attribute of every node id, kept on the device as CSR (tsh_tags_create): entry i of `lists` is the
  /// set of node id i -- the group ids of an ACL, tags, labels; strings go in through a dictionary of the caller's.  A
  /// list that holds [HipRowAttr.nullValue] makes the row a NULL row, as a row beyond `lists` is; an empty list is the
  /// empty set, not NULL.  The column crosses the FFI boundary once; [HipTagColumn.set] extends it as rows are appended.
  /// Dispose it before this backend.
  HipTagColumn? createTags(List<List<int>> lists) {
    final csr = HipTagColumn._csr(lists);
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _tagsCreate(_handle, csr.offsets, lists.length, csr.values, out.cast<Void>());
      if (rc != 0) {
        Logger.warn('tsh_tags_create failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipTagColumn._(out.value);
    } finally {
      csr.free();
      calloc.free(out);
    }
  }

  /// A mask made ON the device from one HAS ANY / HAS ALL term over a tag column (tsh_mask_create_tags): keeps the node
  /// ids whose set is not NULL and for which (the row holds at least t distinct values of `values`) != negate, t being
  /// the number of distinct values for `need` == [tagsAll], else `need` ([tagsAny] is 1); and-ed (or, with `or: true`,
  /// or-ed) with `withMask` when one is given.  At most [tagsMaxSetValues] distinct values.  `tenant = 7 AND acl HAS ANY
  /// (...)` is [createMaskWhereClauses] and then this call with its mask as `withMask`.  A snapshot, as
  /// [createMaskWhere]'s.  Null on any native failure; a disposed [HipTagColumn] or `withMask` is refused (null, with a
  /// warning), never sent as NULL.
  HipRowMask? createMaskTags(HipTagColumn tags, Int64List values,
      {int need = tagsAny, bool negate = false, HipRowMask? withMask, bool or = false}) {
    if (tags._tags == nullptr) {
      Logger.warn('createMaskTags with a disposed HipTagColumn', label: 'HipVectorBackend');
      return null;
    }
    if (withMask != null && withMask._mask == nullptr) {
      Logger.warn('createMaskTags with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    final buf = calloc<Int64>(values.isEmpty ? 1 : values.length);
    final out = calloc<Pointer<Void>>();
    try {
      buf.asTypedList(values.length).setAll(0, values);
      final rc = _maskCreateTags(
          _handle, tags._tags, buf, values.length, need, negate ? 1 : 0, withMask?._mask ?? nullptr, or ? 1 : 0, out);
      if (rc != 0) {
        Logger.warn('tsh_mask_create_tags failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipRowMask._(out.value);
    } finally {
      calloc.free(buf);
      calloc.free(out);
    }
  }

  /// Facet counts ON the device (tsh_attr_facets / tsh_tags_facets) behind [HipRowAttr.facets] and [HipTagColumn.facets]:
  /// `column` is the handle of either kind, `kind` is [facetValues] or [facetEdges] for an attribute column and null for
  /// a tag column.  Null on any native failure.
  HipFacetCounts? _facets(Pointer<Void> column, int? kind, Int64List keys, HipRowMask? mask) {
    final buf = calloc<Int64>(keys.isEmpty ? 1 : keys.length);
    final counts = calloc<Int64>(keys.isEmpty ? 1 : keys.length);
    final rest = calloc<Int64>(3);
    try {
      buf.asTypedList(keys.length).setAll(0, keys);
      final m = mask?._mask ?? nullptr;
      final rc = kind != null
          ? _attrFacets(_handle, column, m, kind, buf, keys.length, counts, rest)
          : _tagsFacets(_handle, column, m, buf, keys.length, counts, rest);
      if (rc != 0) {
        Logger.warn('${kind != null ? 'tsh_attr_facets' : 'tsh_tags_facets'} failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      return HipFacetCounts(Int64List.fromList(counts.asTypedList(keys.length)), rest[0], rest[1], rest[2]);
    } finally {
      calloc.free(buf);
      calloc.free(counts);
      calloc.free(rest);
    }
  }

  /// TSH_FACET_VALUES / TSH_FACET_EDGES and the limit of one facet call (include/tostore_hip.h).
  static const int facetValues = 0;
  static const int facetEdges = 1;
  static const int facetMaxKeys = 4096;

  /// TSH_TAGS_ALL / TSH_TAGS_ANY and the limit of one tsh_mask_create_tags call (include/tostore_hip.h).
  static const int tagsAll = 0;
  static const int tagsAny = 1;
  static const int tagsMaxSetValues = 4096;

  /// TSH_TERM_RANGE / TSH_TERM_IN and the limits of one tsh_mask_create_where call (include/tostore_hip.h).
  static const int termRange = 0;
  static const int termIn = 1;
  static const int whereMaxTerms = 32;
  static const int whereMaxColumns = 8;
  static const int whereMaxSetValues = 4096;

  int get size => _size(_handle);

  /// Replaces the trainPqSubspace isolate fan-out of _ensurePqCodebook
  /// (vector_index_manager.dart:740-850): same codebook, bit for bit, because the
  /// seeds are drawn here exactly as compute_tasks.dart:2144-2151 draws them.
  static Float32List? trainCodebook(List<Float32List> samples, int dimensions, int subspaces,
      {int iterations = 10}) {
    if (!available || samples.length < 100) return null; // small sets keep VectorQuantizer.train
    final n = samples.length;
    final k = n < 256 ? n : 256;
    final subDim = dimensions ~/ subspaces;
    final pSamples = calloc<Float>(n * dimensions);
    final pInit = calloc<Int32>(subspaces * k);
    final pOut = calloc<Float>(subspaces * k * subDim);
    try {
      final flat = pSamples.asTypedList(n * dimensions);
      for (int i = 0; i < n; i++) {
        flat.setRange(i * dimensions, (i + 1) * dimensions, samples[i]);
      }
      final init = pInit.asTypedList(subspaces * k);
      for (int m = 0; m < subspaces; m++) {
        final random = Random(42 + m);
        for (int c = 0; c < k; c++) {
          init[m * k + c] = random.nextInt(n);
        }
      }
      final rc = _pqTrain(0, pSamples, n, dimensions, subspaces, k, iterations, pInit, pOut);
      if (rc != 0) {
        Logger.warn('tsh_pq_train failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return Float32List.fromList(pOut.asTypedList(subspaces * k * subDim));
    } finally {
      calloc.free(pSamples);
      calloc.free(pInit);
      calloc.free(pOut);
    }
  }

  /// Replaces batchPqEncode (compute_tasks.dart:2292-2326) for rows that are already
  /// resident: n x subspaces code bytes for node ids [firstNodeId, firstNodeId + n).
  Uint8List? pqEncode(int firstNodeId, int n, PqCodebook codebook) {
    final pCb = calloc<Float>(codebook.data.length);
    final pOut = calloc<Uint8>(n * codebook.subspaces);
    try {
      pCb.asTypedList(codebook.data.length).setAll(0, codebook.data);
      final rc = _pqEncode(_handle, firstNodeId, n, pCb, codebook.subspaces,
          codebook.centroids, pOut);
      if (rc != 0) {
        Logger.warn('tsh_index_pq_encode failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      return Uint8List.fromList(pOut.asTypedList(n * codebook.subspaces));
    } finally {
      calloc.free(pCb);
      calloc.free(pOut);
    }
  }

  /// Feed from NghGraphEngine.insertBatch (ngh_graph_engine.dart:297-403): the
  /// Float32Lists produced by prepareVectorBatchChunk, ids dense from `firstNodeId`.
  bool append(int firstNodeId, List<Float32List> vectors) {
    if (vectors.isEmpty) return true;
    final n = vectors.length;
    final buf = calloc<Float>(n * dimensions);
    try {
      final view = buf.asTypedList(n * dimensions);
      for (var i = 0; i < n; i++) {
        view.setRange(i * dimensions, (i + 1) * dimensions, vectors[i]);
      }
      final rc = _append(_handle, firstNodeId, n, buf);
      if (rc != 0) Logger.warn('tsh_index_append failed ($rc): ${_errorText()}');
      return rc == 0;
    } finally {
      calloc.free(buf);
    }
  }

  /// Feed from NghGraphEngine.deleteBatch (ngh_graph_engine.dart:411-445).
  bool setDeleted(List<int> nodeIds) {
    if (nodeIds.isEmpty) return true;
    final buf = calloc<Int64>(nodeIds.length);
    try {
      buf.asTypedList(nodeIds.length).setAll(0, nodeIds);
      return _setDeleted(_handle, buf, nodeIds.length) == 0;
    } finally {
      calloc.free(buf);
    }
  }

  /// Cold load of one rawvec partition file (path_manager.dart:318-324).
  int loadRawVectorFile(String path, NghIndexMeta meta, int firstNodeId, int maxRows) {
    final p = path.toNativeUtf8();
    final out = calloc<Int64>();
    try {
      final rc = _loadRawvec(_handle, p, meta.nghPageSize, meta.precision.index,
          firstNodeId, maxRows, out);
      return rc == 0 ? out.value : -1;
    } finally {
      calloc.free(p);
      calloc.free(out);
    }
  }

  /// Drop-in for NghGraphEngine.search (ngh_graph_engine.dart:67-135).  `query`
  /// is already _toFloat32'ed and (cosine) _normalizeFloat32'ed by the caller
  /// (vector_index_manager.dart:514-520).  Returns null on any native failure so
  /// the caller falls through to the original graph search.
  List<NghSearchResult>? search(Float32List query, int topK,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) {
    // a disposed mask is NULL to the library, which reads NULL as "no filter": refuse it instead
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('search with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return const [];
    final q = calloc<Float>(dimensions);
    final ids = calloc<Int64>(topK);
    final dist = calloc<Double>(topK);
    final cnt = calloc<Int32>();
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = mask != null
          ? _searchMasked(_handle, q, 1, topK, distanceThreshold ?? double.nan, mask._mask,
              ids, dist, cnt)
          : _search(_handle, q, 1, topK, distanceThreshold ?? double.nan, maskBytes,
              ids, dist, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      final n = cnt.value;
      return [
        for (var i = 0; i < n; i++) NghSearchResult(nodeId: ids[i], distance: dist[i])
      ];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(cnt);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// One shard of a row-range partitioned index (one Dart process per GPU): holds node ids
  /// [rowBase, rowBase + rows) on `device`; reported ids are global.
  static HipVectorBackend? tryCreateShard(NghIndexMeta meta, int device, int rowBase, int rows) {
    if (!available) return null;
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _createShard(
          meta.dimensions, meta.distanceMetric.index, rows, device, rowBase, out);
      if (rc != 0) {
        Logger.warn('tsh_index_create_shard failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      return HipVectorBackend._(out.value, meta.dimensions, meta.distanceMetric);
    } finally {
      calloc.free(out);
    }
  }

  /// Searches that may be in flight per handle (tsh_max_inflight).
  static int get maxInflight => available ? _maxInflight() : 0;

  /// The asynchronous form of [search]: the query is enqueued (some 20 microseconds), the isolate goes back
  /// to its event loop while the GPU scans, and the result is collected once tsh_search_ready says
  /// so -- the isolate never blocks for longer than the final copy, whatever the corpus size, which
  /// is what the reference's cooperative scheduling asks of everything on the main isolate (8 ms
  /// client / 50 ms server budget: model/data_store_config.dart:225-230,
  /// core/yield_controller.dart:110-169).  Up to [maxInflight] calls may overlap on one handle; their
  /// scans run back to back and each query's select / re-rank hides behind the next scan.
  /// Returns null on any native failure (TSH_E_BUSY included: the caller falls back to the
  /// synchronous path or the Dart graph search).
  Future<List<NghSearchResult>?> searchAsync(Float32List query, int topK,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) async {
    // (as in [search]: a disposed mask must not become "no filter")
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchAsync with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return const [];
    final q = calloc<Float>(dimensions);
    final ticket = calloc<Int32>();
    Pointer<Uint8> maskBytes = nullptr;
    int t;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      // inputs are consumed before either returns (a mask HANDLE must outlive the ticket)
      final rc = mask != null
          ? _submitMasked(_handle, q, topK, mask._mask, ticket)
          : _submit(_handle, q, topK, maskBytes, ticket);
      if (rc != 0) {
        Logger.warn('tsh_search_submit failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      t = ticket.value;
    } finally {
      calloc.free(q);
      calloc.free(ticket);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
    return _collect(t, topK, distanceThreshold);
  }

  /// Polls a ticket and collects its result (the second half of [searchAsync] and [searchAfterAsync]).
  Future<List<NghSearchResult>?> _collect(int t, int topK, double? distanceThreshold) async {
    // every ticket must be waited exactly once: from here on nothing may return before _wait ran.
    // The first polls yield with a zero delay (a short scan is over by then); after that the isolate sleeps
    // between polls -- a zero-delay timer loop would keep its event loop at 100 % CPU for the whole scan, and
    // several isolates or ranks per container share one CPU quota.
    var polls = 0;
    while (true) {
      final ready = _ready(_handle, t);
      if (ready > 0) break;
      if (ready < 0) {
        // the ticket is not pollable (it still must be waited: _wait reports the error and releases it)
        Logger.warn('tsh_search_ready failed ($ready): ${_errorText()}', label: 'HipVectorBackend');
        break;
      }
      polls++;
      await Future<void>.delayed(
          polls <= 4 ? Duration.zero : Duration(microseconds: polls <= 12 ? 50 : 200));
    }
    final ids = calloc<Int64>(topK);
    final dist = calloc<Double>(topK);
    final cnt = calloc<Int32>();
    try {
      final rc = _wait(_handle, t, distanceThreshold ?? double.nan, ids, dist, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_wait failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      final n = cnt.value;
      return [
        for (var i = 0; i < n; i++) NghSearchResult(nodeId: ids[i], distance: dist[i])
      ];
    } finally {
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(cnt);
    }
  }

  /// The next `topK` rows past a cursor (tsh_search_after; no reference counterpart): the first `topK` entries of
  /// the list [search] would return with topK = infinity -- ordered by distance (double.compareTo), ties by node id,
  /// ngh_graph_engine.dart:122-134 -- that are strictly greater than (`afterDistance`, `afterNodeId`), usually the
  /// last entry of the page before.  `afterDistance` = double.negativeInfinity starts a list.  Successive pages
  /// concatenate to exactly that list; a page shorter than `topK` is the last one; each page costs one scan however
  /// deep it is.  "Every row within distanceThreshold" is a loop of pages.  Null on any native failure.
  List<NghSearchResult>? searchAfter(Float32List query, int topK, double afterDistance, int afterNodeId,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) {
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchAfter with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return const [];
    final q = calloc<Float>(dimensions);
    final ids = calloc<Int64>(topK);
    final dist = calloc<Double>(topK);
    final cnt = calloc<Int32>();
    final aDist = calloc<Double>();
    final aId = calloc<Int64>();
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      aDist.value = afterDistance;
      aId.value = afterNodeId;
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _searchAfter(_handle, q, 1, topK, distanceThreshold ?? double.nan, maskBytes,
          mask != null ? mask._mask : nullptr, aDist, aId, ids, dist, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_after failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      final n = cnt.value;
      return [
        for (var i = 0; i < n; i++) NghSearchResult(nodeId: ids[i], distance: dist[i])
      ];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(cnt);
      calloc.free(aDist);
      calloc.free(aId);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// The asynchronous form of [searchAfter], as [searchAsync] is of [search] (tsh_search_submit_after; the ticket
  /// is polled and waited for like any other).
  Future<List<NghSearchResult>?> searchAfterAsync(
      Float32List query, int topK, double afterDistance, int afterNodeId,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) async {
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchAfterAsync with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return const [];
    final q = calloc<Float>(dimensions);
    final ticket = calloc<Int32>();
    Pointer<Uint8> maskBytes = nullptr;
    int t;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _submitAfter(_handle, q, topK, maskBytes, mask != null ? mask._mask : nullptr,
          afterDistance, afterNodeId, ticket);
      if (rc != 0) {
        Logger.warn('tsh_search_submit_after failed ($rc): ${_errorText()}',
            label: 'HipVectorBackend');
        return null;
      }
      t = ticket.value;
    } finally {
      calloc.free(q);
      calloc.free(ticket);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
    return _collect(t, topK, distanceThreshold);
  }

  /// The cursor searches' counters (tsh_search_after_stats), per shard search: all of them, rows their floor passes
  /// sent to the side list, searches redone with a larger side list, searches answered without a floor pass.
  Map<String, int>? searchAfterStats() {
    final o = calloc<Int64>(4);
    try {
      if (_searchAfterStats(_handle, o) != 0) return null;
      return {'searches': o[0], 'sideRows': o[1], 'redone': o[2], 'noFloor': o[3]};
    } finally {
      calloc.free(o);
    }
  }

  /// How many rows [searchAfter] would return with topK = infinity (tsh_search_count; no reference counterpart):
  /// the length of the list under the same threshold, mask, tombstones and cursor.  Without `afterDistance` the list
  /// is [search]'s; with it (and `afterNodeId`) only the rows strictly past that cursor count, so after any page
  /// `searchCount` of its last entry is what is left.  One scan and a pass over its keys: no page is fetched.
  /// Null on any native failure.
  int? searchCount(Float32List query,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask, double? afterDistance, int afterNodeId = 0}) {
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchCount with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (size == 0) return 0;
    final q = calloc<Float>(dimensions);
    final cnt = calloc<Int64>();
    Pointer<Double> aDist = nullptr;
    Pointer<Int64> aId = nullptr;
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (afterDistance != null) {
        aDist = calloc<Double>();
        aId = calloc<Int64>();
        aDist.value = afterDistance;
        aId.value = afterNodeId;
      }
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _searchCount(_handle, q, 1, distanceThreshold ?? double.nan, maskBytes,
          mask != null ? mask._mask : nullptr, aDist, aId, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_count failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return cnt.value;
    } finally {
      calloc.free(q);
      calloc.free(cnt);
      if (aDist != nullptr) calloc.free(aDist);
      if (aId != nullptr) calloc.free(aId);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// The counts' counters (tsh_search_count_stats), per shard search: all of them, rows their window passes sent to
  /// the side list, counts redone with a larger side list, counts answered without a window pass on the device.
  Map<String, int>? searchCountStats() {
    final o = calloc<Int64>(4);
    try {
      if (_searchCountStats(_handle, o) != 0) return null;
      return {'searches': o[0], 'sideRows': o[1], 'redone': o[2], 'noWindow': o[3]};
    } finally {
      calloc.free(o);
    }
  }

  /// The group of every node id, for [searchGrouped] (tsh_groups_create): entry i of `groupOf` is the group of node
  /// id i -- a document, a video, a product --, at least 0 and below `nGroups`, or negative for a row that stands for
  /// itself; rows beyond the list are ungrouped.  The array crosses the FFI boundary once; [HipRowGroups.set] extends
  /// it as rows are appended.  Dispose it before this backend.
  HipRowGroups? createGroups(Int32List groupOf, int nGroups) {
    final buf = calloc<Int32>(groupOf.isEmpty ? 1 : groupOf.length);
    final out = calloc<Pointer<Void>>();
    try {
      buf.asTypedList(groupOf.length).setAll(0, groupOf);
      final rc = _groupsCreate(_handle, buf, groupOf.length, nGroups, out.cast<Void>());
      if (rc != 0) {
        Logger.warn('tsh_groups_create failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return HipRowGroups._(out.value);
    } finally {
      calloc.free(buf);
      calloc.free(out);
    }
  }

  /// The nearest row of each of the `topK` nearest groups (tsh_search_grouped; no reference counterpart): the list
  /// [search] would return with topK = infinity, every entry dropped whose group occurred earlier in it, cut to topK.
  /// One scan, three passes over its keys and a handful of exact rows -- not one [searchAfter] page per long document.
  /// Null on any native failure; a disposed [HipRowGroups] or [HipRowMask] is refused (null, with a warning), never
  /// sent as NULL.
  List<HipGroupedResult>? searchGrouped(Float32List query, int topK, HipRowGroups groups,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) {
    if (groups._groups == nullptr) {
      Logger.warn('searchGrouped with a disposed HipRowGroups', label: 'HipVectorBackend');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchGrouped with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return <HipGroupedResult>[];
    final q = calloc<Float>(dimensions);
    final ids = calloc<Int64>(topK);
    final dist = calloc<Double>(topK);
    final grp = calloc<Int32>(topK);
    final cnt = calloc<Int32>();
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _searchGrouped(_handle, q, 1, topK, distanceThreshold ?? double.nan, maskBytes,
          mask != null ? mask._mask : nullptr, groups._groups, ids, dist, grp, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_grouped failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return [for (var i = 0; i < cnt.value; ++i) HipGroupedResult(ids[i], dist[i], grp[i])];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(grp);
      calloc.free(cnt);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// The grouped searches' counters (tsh_search_grouped_stats), per shard search: all of them, rows their side passes
  /// sent to the side list, searches redone with a larger side list, searches answered without the device group passes.
  Map<String, int>? searchGroupedStats() {
    final o = calloc<Int64>(4);
    try {
      if (_searchGroupedStats(_handle, o) != 0) return null;
      return {'searches': o[0], 'sideRows': o[1], 'redone': o[2], 'noDevicePasses': o[3]};
    } finally {
      calloc.free(o);
    }
  }

  /// The `groupSize` nearest rows of each of the `topK` nearest groups (tsh_search_grouped_rows; no reference
  /// counterpart): the winning groups are [searchGrouped]'s, in its order, and of each the first `groupSize` entries of
  /// the list [search] would return with topK = infinity, in that list's order -- a document's best passages from the
  /// one scan.  One inner list per group returned; a group with fewer surviving rows gives what it has.  `groupSize`
  /// runs from 1 to 64.  Null on any native failure; a disposed [HipRowGroups] or [HipRowMask] is refused (null, with a
  /// warning), never sent as NULL.
  List<List<HipGroupedResult>>? searchGroupedRows(Float32List query, int topK, int groupSize, HipRowGroups groups,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) {
    if (groups._groups == nullptr) {
      Logger.warn('searchGroupedRows with a disposed HipRowGroups', label: 'HipVectorBackend');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchGroupedRows with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (groupSize < 1 || groupSize > 64) {
      Logger.warn('searchGroupedRows: groupSize $groupSize outside [1, 64]', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return <List<HipGroupedResult>>[];
    final q = calloc<Float>(dimensions);
    final ids = calloc<Int64>(topK * groupSize);
    final dist = calloc<Double>(topK * groupSize);
    final grp = calloc<Int32>(topK);
    final rows = calloc<Int32>(topK);
    final cnt = calloc<Int32>();
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _searchGroupedRows(_handle, q, 1, topK, groupSize, distanceThreshold ?? double.nan, maskBytes,
          mask != null ? mask._mask : nullptr, groups._groups, ids, dist, grp, rows, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_grouped_rows failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return [
        for (var i = 0; i < cnt.value; ++i)
          [for (var j = 0; j < rows[i]; ++j) HipGroupedResult(ids[i * groupSize + j], dist[i * groupSize + j], grp[i])]
      ];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(grp);
      calloc.free(rows);
      calloc.free(cnt);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// The rows-per-group searches' counters (tsh_search_grouped_rows_stats), per shard job: the searches, groups their
  /// mark passes marked, member rows sent on for exact sums, jobs redone with larger lists, jobs answered by the
  /// exact-all route.
  Map<String, int>? searchGroupedRowsStats() {
    final o = calloc<Int64>(5);
    try {
      if (_searchGroupedRowsStats(_handle, o) != 0) return null;
      return {'searches': o[0], 'markedGroups': o[1], 'memberRows': o[2], 'redone': o[3], 'exactAll': o[4]};
    } finally {
      calloc.free(o);
    }
  }

  /// The next `topK` groups past a cursor (tsh_search_grouped_after): the entries of [searchGrouped]'s list that follow
  /// (`afterDistance`, `afterId`) strictly -- the last entry of the page before; double.negativeInfinity starts the list.
  /// A group whose best row is at or before the cursor is consumed: none of its rows comes back.  A page shorter than
  /// topK is the last.  Null on any native failure; a disposed [HipRowGroups] or [HipRowMask] is refused (null, with a
  /// warning), never sent as NULL.
  List<HipGroupedResult>? searchGroupedAfter(Float32List query, int topK, HipRowGroups groups, double afterDistance, int afterId,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) {
    if (groups._groups == nullptr) {
      Logger.warn('searchGroupedAfter with a disposed HipRowGroups', label: 'HipVectorBackend');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchGroupedAfter with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (topK <= 0 || size == 0) return <HipGroupedResult>[];
    final q = calloc<Float>(dimensions);
    final ids = calloc<Int64>(topK);
    final dist = calloc<Double>(topK);
    final grp = calloc<Int32>(topK);
    final cnt = calloc<Int32>();
    final aDist = calloc<Double>();
    final aId = calloc<Int64>();
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      aDist.value = afterDistance;
      aId.value = afterId;
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _searchGroupedAfter(_handle, q, 1, topK, distanceThreshold ?? double.nan, maskBytes,
          mask != null ? mask._mask : nullptr, groups._groups, aDist, aId, ids, dist, grp, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_grouped_after failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return [for (var i = 0; i < cnt.value; ++i) HipGroupedResult(ids[i], dist[i], grp[i])];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(grp);
      calloc.free(cnt);
      calloc.free(aDist);
      calloc.free(aId);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// How many groups [searchGroupedAfter] would return with topK = infinity (tsh_search_grouped_count): with
  /// `afterDistance` null, the whole grouped list.  Null on any native failure or a disposed handle.
  int? countGroups(Float32List query, HipRowGroups groups,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask, double? afterDistance, int afterId = 0}) {
    if (groups._groups == nullptr) {
      Logger.warn('countGroups with a disposed HipRowGroups', label: 'HipVectorBackend');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('countGroups with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    if (size == 0) return 0;
    final q = calloc<Float>(dimensions);
    final out = calloc<Int64>();
    Pointer<Double> aDist = nullptr;
    Pointer<Int64> aId = nullptr;
    Pointer<Uint8> maskBytes = nullptr;
    try {
      q.asTypedList(dimensions).setAll(0, query);
      if (afterDistance != null) {
        aDist = calloc<Double>();
        aId = calloc<Int64>();
        aDist.value = afterDistance;
        aId.value = afterId;
      }
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = _searchGroupedCount(_handle, q, 1, distanceThreshold ?? double.nan, maskBytes,
          mask != null ? mask._mask : nullptr, groups._groups, aDist, aId, out);
      if (rc != 0) {
        Logger.warn('tsh_search_grouped_count failed ($rc): ${_errorText()}', label: 'HipVectorBackend');
        return null;
      }
      return out.value;
    } finally {
      calloc.free(q);
      calloc.free(out);
      if (aDist != nullptr) calloc.free(aDist);
      if (aId != nullptr) calloc.free(aId);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  /// The grouped cursor searches' and group counts' counters (tsh_search_grouped_after_stats), per shard job: the
  /// searches, the counts, rows sent to the side list, jobs redone with a larger side list, jobs answered by the
  /// exact-all route.
  Map<String, int>? searchGroupedAfterStats() {
    final o = calloc<Int64>(5);
    try {
      if (_searchGroupedAfterStats(_handle, o) != 0) return null;
      return {'searches': o[0], 'counts': o[1], 'sideRows': o[2], 'redone': o[3], 'exactAll': o[4]};
    } finally {
      calloc.free(o);
    }
  }

  /// Diagnostics for Logger (handler/logger.dart:8-60): rows, searches, candidates per query,
  /// resident bytes, safe mode / quarantined rows.
  Map<String, num>? counters() {
    final c = calloc<TshCounters>();
    try {
      if (_counters(_handle, c) != 0) return null;
      final r = c.ref;
      return {
        'rows': r.rows,
        'deletedRows': r.deletedRows,
        'searches': r.searches,
        'scanLaunches': r.scanLaunches,
        'batchLaunches': r.batchLaunches,
        'fallbackSearches': r.fallbackSearches,
        'candidatesTotal': r.candidatesTotal,
        'bytesResident': r.bytesResident,
        'safeMode': r.safeMode,
        'deviceId': r.deviceId,
        'quarantinedRows': r.quarantinedRows,
        'batchKernelLast': r.batchKernelLast,
        'batchPlaneFallbacks': r.batchPlaneFallbacks,
        'batchScanFallbacks': r.batchScanFallbacks,
        'listScans': r.listScans,
        'exactScans': r.exactScans,
        'exactRedone': r.exactRedone,
      };
    } finally {
      calloc.free(c);
    }
  }

  /// tsh_index_set_option: 1 = TSH_OPT_BATCH_MIN_NQ, 2 = TSH_OPT_BATCH_KERNEL, 4 = TSH_OPT_EXACT_SCAN_ROWS,
  /// 5 = TSH_OPT_EXACT_SELECT, 6 = TSH_OPT_BATCH_HUB, 7 = TSH_OPT_BATCH_GROUP, 8 = TSH_OPT_SCAN_F16,
  /// 9 = TSH_OPT_SCAN_F16_MASKED, 10 = TSH_OPT_SCAN_I8, 12 = TSH_OPT_SCAN_STREAMS, 13 = TSH_OPT_SCAN_I8_MASKED,
  /// 14 = TSH_OPT_SCAN_I4 (tuning only: results never depend on them).
  bool setOption(int option, int value) => _setOption(_handle, option, value) == 0;

  /// TSH_OPT_SCAN_I8_MASKED: the int8 coarse pass behind row masks, tombstones, quarantined rows and gaps -- 0 never,
  /// 1 auto (shards above 256 MiB; gives way to a forced fp16 masked route), 2 every eligible masked scan.
  static const int optScanI8Masked = 13;
  bool setScanI8Masked(int mode) => setOption(optScanI8Masked, mode);

  /// TSH_OPT_SCAN_I4: a 4-bit first pass in front of the dense L2 int8 scan -- 0 never, 1 auto (L2 shards above
  /// 1400 MiB), 2 every eligible scan.
  static const int optScanI4 = 14;
  bool setScanI4(int mode) => setOption(optScanI4, mode);

  /// The fp16 scan's counters (TSH_OPT_SCAN_F16): scans over the fp16 copy of the rows, queries redone through the
  /// f32 scan, rows converted, bytes of the copy resident.
  Map<String, int>? scanF16Stats() {
    final o = calloc<Int64>(4);
    try {
      if (_scanF16Stats(_handle, o) != 0) return null;
      return {'scans': o[0], 'redone': o[1], 'rowsConverted': o[2], 'copyBytes': o[3]};
    } finally {
      calloc.free(o);
    }
  }

  /// Diagnostics: the fp16 scan's stored key (upper side of its band) and band of every row for one query;
  /// `keys` and `w` hold one float per row.
  bool probeScanF16Keys(Pointer<Float> query, Pointer<Float> keys, Pointer<Float> w) =>
      _probeScanF16(_handle, query, keys, w) == 0;

  /// The int8 scan's counters (TSH_OPT_SCAN_I8): scans over the int8 copy of the rows, queries redone through the
  /// f32 scan, rows converted, bytes of the copy resident.
  Map<String, int>? scanI8Stats() {
    final o = calloc<Int64>(4);
    try {
      if (_scanI8Stats(_handle, o) != 0) return null;
      return {'scans': o[0], 'redone': o[1], 'rowsConverted': o[2], 'copyBytes': o[3]};
    } finally {
      calloc.free(o);
    }
  }

  /// Diagnostics: the two sides of the int8 scan's band around every row's key for one query; `lower` and `upper`
  /// hold one float per row.
  bool probeScanI8Keys(Pointer<Float> query, Pointer<Float> lower, Pointer<Float> upper) =>
      _probeScanI8(_handle, query, lower, upper) == 0;

  /// The 4-bit first pass's counters (TSH_OPT_SCAN_I4): scans it ran in, rows it left to the int8 scan, rows converted,
  /// bytes of the plane, times the route was denied, eligible scans a denial still covers.
  Map<String, int>? scanI4Stats() {
    final o = calloc<Int64>(6);
    try {
      if (_scanI4Stats(_handle, o) != 0) return null;
      return {'scans': o[0], 'survivors': o[1], 'rowsConverted': o[2], 'copyBytes': o[3], 'denials': o[4], 'deniedLeft': o[5]};
    } finally {
      calloc.free(o);
    }
  }

  /// Diagnostics: the two sides of the 4-bit pass's band around every row's key for one query; `lower` and `upper`
  /// hold one float per row.
  bool probeScanI4Keys(Pointer<Float> query, Pointer<Float> lower, Pointer<Float> upper) =>
      _probeScanI4(_handle, query, lower, upper) == 0;

  int get nativeDimensions => _dim(_handle);
  int get nativeMetric => _metric(_handle);

  /// Row-sharded deployments whose exchange the HOST does itself (any transport): this shard's
  /// candidate blocks for `queries` into `deviceBlocks` (device memory of
  /// nq * candidateBlockBytes(entries) bytes), to be gathered from all ranks and merged with
  /// [mergeCandidates].  Hosts on one node use [HipShardComm] instead, which does all of it.
  static int candidateBlockBytes(int entries) => _blockBytes(entries);
  static int defaultBlockEntries(int k) => _blockEntries(k);
  bool searchShard(Pointer<Float> queries, int nq, int topK, Pointer<Uint8> rowMask, int entries,
          Pointer<Void> deviceBlocks) =>
      _searchShard(_handle, queries, nq, topK, rowMask, entries, deviceBlocks, nullptr) == 0;

  /// Progressive form (tsh_search_shard_begin / _progress / _end): the scans of all `nq` queries run as one
  /// pipeline on a library thread while the host exchanges the groups whose blocks are final.  Returns the
  /// stream handle (nullptr on failure); `step` = the host's group size.  The queries / mask are copied by the
  /// call; `deviceBlocks` must stay valid until [shardStreamEnd].
  Pointer<Void> shardStreamBegin(Pointer<Float> queries, int nq, int topK, Pointer<Uint8> rowMask,
      int entries, Pointer<Void> deviceBlocks, int step) {
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _shardBegin(_handle, queries, nq, topK, rowMask, entries, deviceBlocks, step, out);
      return rc == 0 ? out.value : nullptr;
    } finally {
      calloc.free(out);
    }
  }

  /// Blocks until the first min(want, nq) queries' blocks are final; -1 when the search failed first,
  /// otherwise the number of leading queries that are final.
  static int shardStreamProgress(Pointer<Void> stream, int want) {
    final done = calloc<Int32>();
    try {
      return _shardProgress(stream, want, done) == 0 ? done.value : -1;
    } finally {
      calloc.free(done);
    }
  }

  /// Waits for whatever still runs and frees the stream; exactly once per [shardStreamBegin].
  static bool shardStreamEnd(Pointer<Void> stream) => _shardEnd(stream) == 0;

  /// Host-side merge of `nBlocks` x nq gathered candidate blocks; false with `neededEntries`
  /// set when a block was truncated (every rank retries with that many entries).
  static bool mergeCandidates(int metric, int dim, Pointer<Float> queries, int nq, int topK,
      double? distanceThreshold, Pointer<Void> blocks, int nBlocks, int entries,
      Pointer<Int64> outIds, Pointer<Double> outDist, Pointer<Int32> outCount,
      Pointer<Int32> neededEntries) {
    return _merge(metric, dim, queries, nq, topK, distanceThreshold ?? double.nan, blocks, nBlocks,
            entries, outIds, outDist, outCount, neededEntries) ==
        0;
  }

  /// The same three behind a GLOBAL cursor per query (`afterDist` / `afterId`: nq each, the same on every rank;
  /// -inf = from the start): every shard's block holds the rows that can be among ITS next topK past the cursor,
  /// and the merge drops what is at or before the exact (distance, id) -- pages concatenate to the list the
  /// cursor-less merge would return with topK = infinity (tsh_search_shard_after, tsh_search_shard_begin_after,
  /// tsh_merge_candidates_after).  [shardStreamProgress] / [shardStreamEnd] serve [shardStreamBeginAfter] too.
  bool searchShardAfter(Pointer<Float> queries, int nq, int topK, Pointer<Uint8> rowMask,
          Pointer<Double> afterDist, Pointer<Int64> afterId, int entries, Pointer<Void> deviceBlocks) =>
      _searchShardAfter(_handle, queries, nq, topK, rowMask, afterDist, afterId, entries, deviceBlocks, nullptr) == 0;

  Pointer<Void> shardStreamBeginAfter(Pointer<Float> queries, int nq, int topK, Pointer<Uint8> rowMask,
      Pointer<Double> afterDist, Pointer<Int64> afterId, int entries, Pointer<Void> deviceBlocks, int step) {
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _shardBeginAfter(
          _handle, queries, nq, topK, rowMask, afterDist, afterId, entries, deviceBlocks, step, out);
      return rc == 0 ? out.value : nullptr;
    } finally {
      calloc.free(out);
    }
  }

  static bool mergeCandidatesAfter(int metric, int dim, Pointer<Float> queries, int nq, int topK,
      double? distanceThreshold, Pointer<Double> afterDist, Pointer<Int64> afterId, Pointer<Void> blocks,
      int nBlocks, int entries, Pointer<Int64> outIds, Pointer<Double> outDist, Pointer<Int32> outCount,
      Pointer<Int32> neededEntries) {
    return _mergeAfter(metric, dim, queries, nq, topK, distanceThreshold ?? double.nan, afterDist, afterId,
            blocks, nBlocks, entries, outIds, outDist, outCount, neededEntries) ==
        0;
  }

  /// The same three for the plain grouped search (tsh_search_shard_grouped, tsh_search_shard_begin_grouped,
  /// tsh_merge_candidates_grouped): every shard's block holds its group heads' candidates, the side rows and the
  /// quarantined rows the mask keeps, and the merge -- the grouped finaliser over the union of all blocks -- gives
  /// bit for bit what [searchGrouped] gives on one un-sharded index; groups may have rows on any number of ranks.
  /// `groups`: made by [createGroups] on THIS backend from the same GLOBAL array every rank uses; `rowMask` / `mask`:
  /// GLOBAL, at most one.  A disposed [HipRowGroups] or [HipRowMask] is refused (false / nullptr, with a warning).
  /// [shardStreamProgress] / [shardStreamEnd] serve [shardStreamBeginGrouped] too; the handles must stay undisposed
  /// until [shardStreamEnd].
  bool searchShardGrouped(Pointer<Float> queries, int nq, int topK, Pointer<Uint8> rowMask, HipRowMask? mask,
      HipRowGroups groups, int entries, Pointer<Void> deviceBlocks) {
    if (groups._groups == nullptr) {
      Logger.warn('searchShardGrouped with a disposed HipRowGroups', label: 'HipVectorBackend');
      return false;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchShardGrouped with a disposed HipRowMask', label: 'HipVectorBackend');
      return false;
    }
    return _searchShardGrouped(_handle, queries, nq, topK, rowMask, mask?._mask ?? nullptr, groups._groups, entries,
            deviceBlocks, nullptr) ==
        0;
  }

  Pointer<Void> shardStreamBeginGrouped(Pointer<Float> queries, int nq, int topK, Pointer<Uint8> rowMask,
      HipRowMask? mask, HipRowGroups groups, int entries, Pointer<Void> deviceBlocks, int step) {
    if (groups._groups == nullptr) {
      Logger.warn('shardStreamBeginGrouped with a disposed HipRowGroups', label: 'HipVectorBackend');
      return nullptr;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('shardStreamBeginGrouped with a disposed HipRowMask', label: 'HipVectorBackend');
      return nullptr;
    }
    final out = calloc<Pointer<Void>>();
    try {
      final rc = _shardBeginGrouped(_handle, queries, nq, topK, rowMask, mask?._mask ?? nullptr, groups._groups,
          entries, deviceBlocks, step, out);
      return rc == 0 ? out.value : nullptr;
    } finally {
      calloc.free(out);
    }
  }

  /// `groupOf` / `nGroupOf`: the GLOBAL array the ranks' [HipRowGroups] were made from; `outGroup` may be nullptr.
  static bool mergeCandidatesGrouped(int metric, int dim, Pointer<Float> queries, int nq, int topK,
      double? distanceThreshold, Pointer<Int32> groupOf, int nGroupOf, Pointer<Void> blocks, int nBlocks,
      int entries, Pointer<Int64> outIds, Pointer<Double> outDist, Pointer<Int32> outGroup,
      Pointer<Int32> outCount, Pointer<Int32> neededEntries) {
    return _mergeGrouped(metric, dim, queries, nq, topK, distanceThreshold ?? double.nan, groupOf, nGroupOf,
            blocks, nBlocks, entries, outIds, outDist, outGroup, outCount, neededEntries) ==
        0;
  }

  /// [searchShard] / [shardStreamBegin] with a device-resident WHERE row set in place of the bitmap pointer, and an
  /// optional GLOBAL cursor per query (tsh_search_shard_masked, tsh_search_shard_begin_masked): the library reads
  /// the mask's device words and list in place -- no per-call slice, count, list or copy of a bitmap on this rank.
  /// `mask`: made by [createMask] on THIS backend from the same GLOBAL bitmap every rank uses (null = no filter); it
  /// must stay undisposed until the call returns -- for the progressive form until [shardStreamEnd].  A disposed
  /// mask is refused (false / nullptr, with a warning): it must not become "no filter".  `afterDistances` /
  /// `afterNodeIds`: both (nq each, [searchShardAfter]'s semantics) or neither.  Blocks, overflow protocol,
  /// [shardStreamProgress] / [shardStreamEnd] and the merge are the pointer forms'.
  bool searchShardMasked(Pointer<Float> queries, int nq, int topK, HipRowMask? mask, int entries,
      Pointer<Void> deviceBlocks, {List<double>? afterDistances, List<int>? afterNodeIds}) {
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchShardMasked with a disposed HipRowMask', label: 'HipVectorBackend');
      return false;
    }
    if ((afterDistances == null) != (afterNodeIds == null)) return false;
    if (afterDistances != null && (afterDistances.length != nq || afterNodeIds!.length != nq)) return false;
    Pointer<Double> ad = nullptr;
    Pointer<Int64> ai = nullptr;
    try {
      if (afterDistances != null) {
        ad = calloc<Double>(nq);
        ai = calloc<Int64>(nq);
        ad.asTypedList(nq).setAll(0, afterDistances);
        ai.asTypedList(nq).setAll(0, afterNodeIds!);
      }
      return _searchShardMasked(_handle, queries, nq, topK, mask?._mask ?? nullptr, ad, ai, entries,
              deviceBlocks, nullptr) ==
          0;
    } finally {
      if (ad != nullptr) calloc.free(ad);
      if (ai != nullptr) calloc.free(ai);
    }
  }

  Pointer<Void> shardStreamBeginMasked(Pointer<Float> queries, int nq, int topK, HipRowMask? mask,
      int entries, Pointer<Void> deviceBlocks, int step,
      {List<double>? afterDistances, List<int>? afterNodeIds}) {
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('shardStreamBeginMasked with a disposed HipRowMask', label: 'HipVectorBackend');
      return nullptr;
    }
    if ((afterDistances == null) != (afterNodeIds == null)) return nullptr;
    if (afterDistances != null && (afterDistances.length != nq || afterNodeIds!.length != nq)) return nullptr;
    Pointer<Double> ad = nullptr;
    Pointer<Int64> ai = nullptr;
    final out = calloc<Pointer<Void>>();
    try {
      if (afterDistances != null) {  // (the cursors are copied by the call, like the queries)
        ad = calloc<Double>(nq);
        ai = calloc<Int64>(nq);
        ad.asTypedList(nq).setAll(0, afterDistances);
        ai.asTypedList(nq).setAll(0, afterNodeIds!);
      }
      final rc = _shardBeginMasked(_handle, queries, nq, topK, mask?._mask ?? nullptr, ad, ai, entries,
          deviceBlocks, step, out);
      return rc == 0 ? out.value : nullptr;
    } finally {
      calloc.free(out);
      if (ad != nullptr) calloc.free(ad);
      if (ai != nullptr) calloc.free(ai);
    }
  }

  void dispose() {
    if (_handle != nullptr) {
      _destroy(_handle);
      _handle = nullptr;
    }
  }
}

/// One rank of a row-sharded index: one Dart process per GPU, the library's own RCCL exchange
/// (tsh_comm_* / tsh_search_sharded).  Rank 0 calls [uniqueId] and ships the 128 bytes to its peers over
/// whatever channel the deployment has; every rank then constructs its communicator (collective) and
/// calls [search] with the same queries (collective).  Every rank gets the full answer.
final class HipShardComm {
  Pointer<Void> _comm;
  final HipVectorBackend shard;

  HipShardComm._(this._comm, this.shard);

  static Uint8List? uniqueId() {
    if (!HipVectorBackend.available) return null;
    final buf = calloc<Uint8>(128);
    try {
      if (HipVectorBackend._commId(buf.cast<Void>()) != 0) return null;
      return Uint8List.fromList(buf.asTypedList(128));
    } finally {
      calloc.free(buf);
    }
  }

  static HipShardComm? tryCreate(
      HipVectorBackend shard, Uint8List id, int world, int rank, int device) {
    if (!HipVectorBackend.available || id.length != 128) return null;
    final buf = calloc<Uint8>(128);
    final out = calloc<Pointer<Void>>();
    try {
      buf.asTypedList(128).setAll(0, id);
      final rc = HipVectorBackend._commCreate(buf.cast<Void>(), world, rank, device, out);
      if (rc != 0) {
        Logger.warn('tsh_comm_create failed ($rc): ${HipVectorBackend._errorText()}',
            label: 'HipShardComm');
        return null;
      }
      return HipShardComm._(out.value, shard);
    } finally {
      calloc.free(buf);
      calloc.free(out);
    }
  }

  /// The same protocol over a transport the host brings (ranks on several nodes): `allgather` is a
  /// `Pointer.fromFunction` / `NativeCallable.isolateLocal` of [TshAllgatherNative] that places every rank's
  /// bytes at recv + rank * bytes on every rank.
  static HipShardComm? tryCreateOverHost(HipVectorBackend shard, int world, int rank, int device,
      Pointer<NativeFunction<TshAllgatherNative>> allgather) {
    if (!HipVectorBackend.available) return null;
    final out = calloc<Pointer<Void>>();
    try {
      final rc =
          HipVectorBackend._commCreateHost(world, rank, device, allgather, nullptr, out);
      if (rc != 0) return null;
      return HipShardComm._(out.value, shard);
    } finally {
      calloc.free(out);
    }
  }

  int get world => HipVectorBackend._commWorld(_comm);

  /// Queries per exchange inside one [search] call (0 = by the size of the call).  Same on every rank.
  bool setGroup(int queriesPerExchange) =>
      HipVectorBackend._commSetGroup(_comm, queriesPerExchange) == 0;

  /// Collective: same queries, topK and threshold on every rank.  null on failure -- this rank's own
  /// (its error is logged) or another rank's (TSH_E_PEER = -11): every rank then takes the same
  /// fallback, and the communicator stays usable.
  List<List<NghSearchResult>>? search(List<Float32List> queries, int topK,
          {double? distanceThreshold, Uint8List? rowMask}) =>
      _search(queries, topK, distanceThreshold, rowMask, null, null);

  /// [search] behind a GLOBAL cursor per query -- the last (distance, nodeId) the caller saw of each; the same
  /// lists on every rank; double.negativeInfinity = from the start: the next topK rows past it, identical on every
  /// rank and equal to what [HipVectorBackend.searchAfter] gives on one un-sharded index over the same rows
  /// (tsh_search_sharded_after).  A page shorter than topK is the last one.
  List<List<NghSearchResult>>? searchShardedAfter(List<Float32List> queries, int topK,
      List<double> afterDistances, List<int> afterNodeIds,
      {double? distanceThreshold, Uint8List? rowMask}) {
    if (afterDistances.length != queries.length || afterNodeIds.length != queries.length) return null;
    return _search(queries, topK, distanceThreshold, rowMask, afterDistances, afterNodeIds);
  }

  /// [search] / [searchShardedAfter] with this rank's device-resident WHERE row set (tsh_search_sharded_masked):
  /// `mask` made by [HipVectorBackend.createMask] on this rank's shard from the same GLOBAL bitmap on every rank
  /// (null = no filter); `afterDistances` / `afterNodeIds`: both or neither.  No rank slices, counts or lists a
  /// bitmap per call.  A disposed mask is refused before the collective is entered (null, with a warning): every
  /// rank must refuse alike, or dispose only between calls.  A mask of another backend is this rank's own failure
  /// inside the collective: its peers get TSH_E_PEER and the communicator stays usable.
  List<List<NghSearchResult>>? searchShardedMasked(List<Float32List> queries, int topK, HipRowMask? mask,
      {double? distanceThreshold, List<double>? afterDistances, List<int>? afterNodeIds}) {
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchShardedMasked with a disposed HipRowMask', label: 'HipShardComm');
      return null;
    }
    if ((afterDistances == null) != (afterNodeIds == null)) return null;
    if (afterDistances != null &&
        (afterDistances.length != queries.length || afterNodeIds!.length != queries.length)) return null;
    return _search(queries, topK, distanceThreshold, null, afterDistances, afterNodeIds,
        handle: mask, viaHandle: true);
  }

  /// [search] for the plain grouped search (tsh_search_sharded_grouped): the nearest row of each of the topK nearest
  /// groups over ALL ranks' rows, identical on every rank and equal to what [HipVectorBackend.searchGrouped] gives on
  /// one un-sharded index.  `groups`: made by [HipVectorBackend.createGroups] on this rank's shard from the same
  /// GLOBAL array on every rank; groups may have rows on any number of ranks.  `rowMask` / `mask`: GLOBAL, at most
  /// one.  A disposed handle is refused before the collective is entered (null, with a warning): every rank must
  /// refuse alike.  A handle of another backend is this rank's own failure inside the collective: its peers get
  /// TSH_E_PEER and the communicator stays usable.
  List<List<HipGroupedResult>>? searchShardedGrouped(List<Float32List> queries, int topK, HipRowGroups groups,
      {double? distanceThreshold, Uint8List? rowMask, HipRowMask? mask}) {
    if (groups._groups == nullptr) {
      Logger.warn('searchShardedGrouped with a disposed HipRowGroups', label: 'HipShardComm');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('searchShardedGrouped with a disposed HipRowMask', label: 'HipShardComm');
      return null;
    }
    final nq = queries.length, d = shard.dimensions;
    if (nq == 0 || topK <= 0) return [for (var i = 0; i < nq; i++) const []];
    final q = calloc<Float>(nq * d);
    final ids = calloc<Int64>(nq * topK);
    final dist = calloc<Double>(nq * topK);
    final grp = calloc<Int32>(nq * topK);
    final cnt = calloc<Int32>(nq);
    Pointer<Uint8> maskBytes = nullptr;
    try {
      final view = q.asTypedList(nq * d);
      for (var i = 0; i < nq; i++) {
        view.setRange(i * d, (i + 1) * d, queries[i]);
      }
      if (mask == null && rowMask != null) {
        maskBytes = calloc<Uint8>(rowMask.length);
        maskBytes.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      final rc = HipVectorBackend._searchShardedGrouped(shard._handle, _comm, q, nq, topK,
          distanceThreshold ?? double.nan, maskBytes, mask?._mask ?? nullptr, groups._groups, ids, dist, grp, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_sharded_grouped failed ($rc): ${HipVectorBackend._errorText()}',
            label: 'HipShardComm');
        return null;
      }
      return [
        for (var i = 0; i < nq; i++)
          [
            for (var j = 0; j < cnt[i]; j++)
              HipGroupedResult(ids[i * topK + j], dist[i * topK + j], grp[i * topK + j])
          ]
      ];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(grp);
      calloc.free(cnt);
      if (maskBytes != nullptr) calloc.free(maskBytes);
    }
  }

  List<List<NghSearchResult>>? _search(List<Float32List> queries, int topK, double? distanceThreshold,
      Uint8List? rowMask, List<double>? afterDistances, List<int>? afterNodeIds,
      {HipRowMask? handle, bool viaHandle = false}) {
    final nq = queries.length, d = shard.dimensions;
    if (nq == 0 || topK <= 0) return [for (var i = 0; i < nq; i++) const []];
    final q = calloc<Float>(nq * d);
    Pointer<Double> ad = nullptr;
    Pointer<Int64> ai = nullptr;
    final ids = calloc<Int64>(nq * topK);
    final dist = calloc<Double>(nq * topK);
    final cnt = calloc<Int32>(nq);
    Pointer<Uint8> mask = nullptr;
    try {
      final view = q.asTypedList(nq * d);
      for (var i = 0; i < nq; i++) {
        view.setRange(i * d, (i + 1) * d, queries[i]);
      }
      if (rowMask != null) {
        mask = calloc<Uint8>(rowMask.length);
        mask.asTypedList(rowMask.length).setAll(0, rowMask);
      }
      if (afterDistances != null && afterNodeIds != null) {
        ad = calloc<Double>(nq);
        ai = calloc<Int64>(nq);
        ad.asTypedList(nq).setAll(0, afterDistances);
        ai.asTypedList(nq).setAll(0, afterNodeIds);
      }
      final rc = viaHandle
          ? HipVectorBackend._searchShardedMasked(shard._handle, _comm, q, nq, topK,
              distanceThreshold ?? double.nan, handle?._mask ?? nullptr, ad, ai, ids, dist, cnt)
          : ad != nullptr
          ? HipVectorBackend._searchShardedAfter(shard._handle, _comm, q, nq, topK,
              distanceThreshold ?? double.nan, mask, ad, ai, ids, dist, cnt)
          : HipVectorBackend._searchSharded(shard._handle, _comm, q, nq, topK,
              distanceThreshold ?? double.nan, mask, ids, dist, cnt);
      if (rc != 0) {
        Logger.warn('tsh_search_sharded failed ($rc): ${HipVectorBackend._errorText()}',
            label: 'HipShardComm');
        return null;
      }
      return [
        for (var i = 0; i < nq; i++)
          [
            for (var j = 0; j < cnt[i]; j++)
              NghSearchResult(nodeId: ids[i * topK + j], distance: dist[i * topK + j])
          ]
      ];
    } finally {
      calloc.free(q);
      calloc.free(ids);
      calloc.free(dist);
      calloc.free(cnt);
      if (mask != nullptr) calloc.free(mask);
      if (ad != nullptr) calloc.free(ad);
      if (ai != nullptr) calloc.free(ai);
    }
  }

  /// Where this rank's [search] time went, summed over the calls so far (tsh_comm_timeline): microseconds per
  /// phase, for Logger diagnostics of a slow multi-GPU deployment.  `reset` starts a new period.
  Map<String, num>? timeline({bool reset = false}) {
    final t = calloc<TshCommTimeline>();
    try {
      if (HipVectorBackend._commTimeline(_comm, t, reset ? 1 : 0) != 0) return null;
      final r = t.ref;
      return {
        'calls': r.calls,
        'queries': r.queries,
        'groups': r.groups,
        'retries': r.retries,
        'world': r.world,
        'rank': r.rank,
        'transport': r.transport,
        'callUs': r.callUs,
        'reserveUs': r.reserveUs,
        'waitScanUs': r.waitScanUs,
        'scanUs': r.scanUs,
        'exchangeWaitUs': r.exchangeWaitUs,
        'gatherUs': r.gatherUs,
        'sliceD2hUs': r.sliceD2hUs,
        'mergeUs': r.mergeUs,
        'resultGatherUs': r.resultGatherUs,
        'copyOutUs': r.copyOutUs,
        'retryScanUs': r.retryScanUs,
        'preEnqueueUs': r.preEnqueueUs,
      };
    } finally {
      calloc.free(t);
    }
  }

  void dispose() {
    if (_comm != nullptr) {
      HipVectorBackend._commDestroy(_comm);
      _comm = nullptr;
    }
  }
}

/// A device-resident WHERE row set ([HipVectorBackend.createMask], tsh_mask_create): the rows a structured
/// filter keeps -- primary keys mapped to node ids through the pk -> nodeId tree
/// (vector_index_manager.dart:1223-1378) -- or the complement of a tombstone set (ngh_page.dart:105-108),
/// kept for as many queries as it serves.  Rows appended after it was made are not kept; rows deleted
/// later are dropped by the kernels as always.  Dispose it before its backend, and only after every
/// [HipVectorBackend.searchAsync] that used it has completed.  A disposed mask is refused by [HipVectorBackend.search]
/// and [HipVectorBackend.searchAsync] (null, with a warning); one whose backend was disposed first is orphaned by the
/// library ([kept] answers -1) and still safe to dispose.
final class HipRowMask {
  Pointer<Void> _mask;

  HipRowMask._(this._mask);

  /// Rows the mask keeps among the index's current node ids (tombstones not subtracted); -1 on failure.
  int get kept => _mask == nullptr ? -1 : HipVectorBackend._maskKept(_mask);

  /// [HipVectorBackend.createMaskWhere] by its other name: the mask of one range term over an attribute column.
  static HipRowMask? where(HipVectorBackend backend, HipRowAttr attr, int lo, int hi,
          {bool negate = false, HipRowMask? withMask, bool or = false}) =>
      backend.createMaskWhere(attr, lo, hi, negate: negate, withMask: withMask, or: or);

  /// [HipVectorBackend.createMaskWhereClauses] by its other name: the mask of a whole WHERE, made in one launch.
  static HipRowMask? whereClauses(HipVectorBackend backend, List<List<HipWhereTerm>> clauses,
          {HipRowMask? withMask, bool or = false}) =>
      backend.createMaskWhereClauses(clauses, withMask: withMask, or: or);

  /// [HipVectorBackend.createMaskTags] by its other name: the mask of one HAS ANY / HAS ALL term over a tag column.
  static HipRowMask? hasTags(HipVectorBackend backend, HipTagColumn tags, Int64List values,
          {int need = HipVectorBackend.tagsAny, bool negate = false, HipRowMask? withMask, bool or = false}) =>
      backend.createMaskTags(tags, values, need: need, negate: negate, withMask: withMask, or: or);

  /// The first `nBytes` bytes of the mask's bitmap as it stands (tsh_mask_read): bit i (LSB first) = node id i, bytes
  /// past what the mask knows read 0.  Null on failure, or on a disposed mask.
  Uint8List? readBits(int nBytes) {
    if (_mask == nullptr || nBytes < 0) return null;
    final buf = calloc<Uint8>(nBytes == 0 ? 1 : nBytes);
    try {
      if (HipVectorBackend._maskRead(_mask, buf, nBytes) != 0) return null;
      return Uint8List.fromList(buf.asTypedList(nBytes));
    } finally {
      calloc.free(buf);
    }
  }

  void dispose() {
    if (_mask != nullptr) {
      HipVectorBackend._maskDestroy(_mask);
      _mask = nullptr;
    }
  }
}

/// One scalar attribute of every node id ([HipVectorBackend.createAttr], tsh_attr_create), kept on the device for as
/// many [HipVectorBackend.createMaskWhere] calls as it serves.  [set] extends or overwrites a range of entries, the
/// companion of the append feed.  Dispose it before its backend; a disposed handle is refused by
/// [HipVectorBackend.createMaskWhere] (null, with a warning), and one whose backend was disposed first is orphaned by
/// the library and still safe to dispose.  Masks made from it outlive it.
final class HipRowAttr {
  Pointer<Void> _attr;

  HipRowAttr._(this._attr);

  /// TSH_ATTR_NULL: the row has no value, and no term keeps it.
  static const int nullValue = -9223372036854775808;

  /// The int64 key of a double column's value (a DateTime's microseconds need none: they are ints): ordered as
  /// double.compareTo orders the values, -0.0 before 0.0 and NaN last, and never [nullValue].
  static int doubleKey(double v) {
    if (v.isNaN) return 0x7FF8000000000000;
    final b = (ByteData(8)..setFloat64(0, v)).getInt64(0);
    return b >= 0 ? b : b ^ 0x7FFFFFFFFFFFFFFF;
  }

  /// Entries [firstNodeId, firstNodeId + values.length) of the column; false on failure (or on a disposed handle).
  bool set(int firstNodeId, Int64List values) {
    if (_attr == nullptr) return false;
    final buf = calloc<Int64>(values.isEmpty ? 1 : values.length);
    try {
      buf.asTypedList(values.length).setAll(0, values);
      return HipVectorBackend._attrSet(_attr, firstNodeId, values.length, buf) == 0;
    } finally {
      calloc.free(buf);
    }
  }

  /// Facet counts over the node ids a search under `mask` could return (tsh_attr_facets): counts[j] = the rows whose
  /// value == keys[j] (keys in any order), or with `edges: true` the rows with keys[j] <= value < keys[j + 1], the last
  /// bucket open and the keys strictly ascending; beside them the rows in no bucket, the rows without a value and all of
  /// them.  At most [HipVectorBackend.facetMaxKeys] distinct keys.  The column is read as it stands: no snapshot.  Null
  /// on any native failure; a disposed column or `mask` is refused (null, with a warning), never sent as NULL.
  HipFacetCounts? facets(HipVectorBackend backend, Int64List keys, {HipRowMask? mask, bool edges = false}) {
    if (_attr == nullptr) {
      Logger.warn('facets with a disposed HipRowAttr', label: 'HipVectorBackend');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('facets with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    return backend._facets(_attr, edges ? HipVectorBackend.facetEdges : HipVectorBackend.facetValues, keys, mask);
  }

  void dispose() {
    if (_attr != nullptr) {
      HipVectorBackend._attrDestroy(_attr);
      _attr = nullptr;
    }
  }
}

/// A caller's lists as the native CSR: `offsets` (lists.length + 1 entries from 0) and `values`, both on the C heap.
final class _TagCsr {
  final Pointer<Int64> offsets;
  final Pointer<Int64> values;
  _TagCsr(this.offsets, this.values);

  void free() {
    calloc.free(offsets);
    calloc.free(values);
  }
}

/// One array-valued attribute of every node id ([HipVectorBackend.createTags], tsh_tags_create), kept on the device as
/// CSR for as many [HipVectorBackend.createMaskTags] calls as it serves.  [set] overwrites or extends a range of rows,
/// the companion of the append feed.  Dispose it before its backend; a disposed column is refused by
/// [HipVectorBackend.createMaskTags] (null, with a warning), and one whose backend was disposed first is orphaned by
/// the library and still safe to dispose.  Masks made from it outlive it.
final class HipTagColumn {
  Pointer<Void> _tags;

  HipTagColumn._(this._tags);

  static _TagCsr _csr(List<List<int>> lists) {
    var total = 0;
    for (final l in lists) {
      total += l.length;
    }
    final offsets = calloc<Int64>(lists.length + 1);
    final values = calloc<Int64>(total == 0 ? 1 : total);
    var at = 0;
    for (var i = 0; i < lists.length; i++) {
      for (final v in lists[i]) {
        values[at++] = v;
      }
      offsets[i + 1] = at;
    }
    return _TagCsr(offsets, values);
  }

  /// Rows [firstNodeId, firstNodeId + lists.length) of the column; rows between its old end and firstNodeId become NULL
  /// rows.  False on failure (or on a disposed column).
  bool set(int firstNodeId, List<List<int>> lists) {
    if (_tags == nullptr) return false;
    final csr = _csr(lists);
    try {
      return HipVectorBackend._tagsSet(_tags, firstNodeId, lists.length, csr.offsets, csr.values) == 0;
    } finally {
      csr.free();
    }
  }

  /// Facet counts over the node ids a search under `mask` could return (tsh_tags_facets): counts[j] = the rows whose set
  /// is not NULL and holds keys[j]; beside them the non-NULL rows that hold none of the keys (empty sets included), the
  /// NULL rows and all of them.  At most [HipVectorBackend.facetMaxKeys] distinct keys.  Null on any native failure; a
  /// disposed column or `mask` is refused (null, with a warning), never sent as NULL.
  HipFacetCounts? facets(HipVectorBackend backend, Int64List keys, {HipRowMask? mask}) {
    if (_tags == nullptr) {
      Logger.warn('facets with a disposed HipTagColumn', label: 'HipVectorBackend');
      return null;
    }
    if (mask != null && mask._mask == nullptr) {
      Logger.warn('facets with a disposed HipRowMask', label: 'HipVectorBackend');
      return null;
    }
    return backend._facets(_tags, null, keys, mask);
  }

  void dispose() {
    if (_tags != nullptr) {
      HipVectorBackend._tagsDestroy(_tags);
      _tags = nullptr;
    }
  }
}

/// What [HipRowAttr.facets] and [HipTagColumn.facets] answer: `counts[j]` for every key as given, then the rows in no
/// bucket, the rows without a value, and all the rows a search under the same mask could return.
final class HipFacetCounts {
  final Int64List counts;
  final int other;
  final int nulls;
  final int total;
  const HipFacetCounts(this.counts, this.other, this.nulls, this.total);
}

/// One entry of [HipVectorBackend.searchGrouped]: a group's nearest row; `group` is -1 for a row that stands for itself.
final class HipGroupedResult {
  final int nodeId;
  final double distance;
  final int group;
  const HipGroupedResult(this.nodeId, this.distance, this.group);
}

/// The group of every node id ([HipVectorBackend.createGroups], tsh_groups_create), kept by the library for as many
/// grouped searches as it serves.  [set] extends or overwrites a range of entries, the companion of the append feed.
/// Dispose it before its backend; a disposed handle is refused by [HipVectorBackend.searchGrouped] (null, with a
/// warning), and one whose backend was disposed first is orphaned by the library and still safe to dispose.
final class HipRowGroups {
  Pointer<Void> _groups;

  HipRowGroups._(this._groups);

  /// Entries [firstNodeId, firstNodeId + groupOf.length) of the array; false on failure (or on a disposed handle).
  bool set(int firstNodeId, Int32List groupOf) {
    if (_groups == nullptr) return false;
    final buf = calloc<Int32>(groupOf.isEmpty ? 1 : groupOf.length);
    try {
      buf.asTypedList(groupOf.length).setAll(0, groupOf);
      return HipVectorBackend._groupsSet(_groups, firstNodeId, groupOf.length, buf) == 0;
    } finally {
      calloc.free(buf);
    }
  }

  void dispose() {
    if (_groups != nullptr) {
      HipVectorBackend._groupsDestroy(_groups);
      _groups = nullptr;
    }
  }
}
