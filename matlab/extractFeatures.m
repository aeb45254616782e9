function [features, validPoints] = extractFeatures(I, points, varargin)
%EXTRACTFEATURES libvo (MI355X) shadow for extractFeatures(I, points, "Method", "SIFT").
%   [features, validPoints] = extractFeatures(I, points, "Method", "SIFT")
%   reference call site: VO.m:83-84.  Returns the N x 128 single descriptors
%   the detectSIFTFeatures shadow computed for these points of this image in
%   the same device pass; every point gets a descriptor (validPoints = points).
%   points may be any subset or permutation of those detections, e.g.
%   selectStrongest(points, N); vo_mex('strongest', N) selects on the device instead.
    if numel(varargin) ~= 2 || ~strcmpi(string(varargin{1}), "Method") || ~strcmpi(string(varargin{2}), "SIFT")
        error('vo:extractFeatures:options', 'libvo implements extractFeatures(I, points, "Method", "SIFT") only');
    end
    if ~isa(I, 'uint8')
        I = im2uint8(I);
    end
    key = [points.Location, points.Scale, points.Orientation];
    desc = vo_sift_cache('get', I, key);
    if isempty(desc) && points.Count > 0   % not among the last detections of this image: detect again
        [loc, scale, ori, ~, all_desc] = vo_mex('sift', I);
        [found, row] = ismember(key, [loc, scale, ori], 'rows');
        if ~all(found)
            error('vo:extractFeatures:points', 'libvo describes the points its own detectSIFTFeatures returned');
        end
        desc = all_desc(row, :);
    end
    features = desc;
    validPoints = points;
end
